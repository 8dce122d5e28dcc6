// Multi-tensor kernels for the gradient path: fused SGD-momentum, bucket pack/unpack
// (tensor fusion), in-place scale.
//
// Reference behaviour being replaced:
//   * pack   = Group.fuse          /root/reference/src/ourdist.py:28-36 (one torch copy per grad)
//   * unpack = Group.unfuse        /root/reference/src/ourdist.py:38-43
//   * average= `send /= size`      /root/reference/src/allreduce.py:98
//   * SGD    = optim.SGD(lr=0.01, momentum=0.5) /root/reference/src/main.py:36,91
//
// Design (MI355X): every op is ONE launch over a device-resident tensor table. The table is
// built once on the host (parameters and bucket layouts are static), so a training step issues
// a single kernel per op regardless of the 161 (ResNet-50) / 467 (ResNet-152) tensors.
// Each 256-thread workgroup owns a 4096-element chunk of one tensor; the tensor is found by a
// binary search over a block-prefix array (≤ 9 steps for 500 tensors). All accesses are 16-byte
// vectors when the tensor is 16-byte aligned (bucket layouts pad every view to 64 B), with a
// scalar tail. These ops are HBM-bound: 12 B/elem read + 8 B/elem written for fp32 SGD; the optional weight
// EMA rides in the list update kernels for 4 B/elem more each way (times: profiles/ema/README.md).
#include "dla_common.h"
#include "dla_kernels.h"

namespace dla {

constexpr int kMTBlock = 256;
constexpr int kMTPerThread = 16;  // 4 x float4
static_assert(kMTChunk == kMTBlock * kMTPerThread, "the host's chunk size is one block's work");

__device__ __forceinline__ int find_tensor(const int32_t* __restrict__ prefix, int ntensors, int block) {
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// This block's work: elements [begin, end) of tensor t, whose entry is e; full = a whole chunk.
template <typename E>
struct Chunk {
  E e;
  int t;
  int64_t begin, end;
  bool full;
};
template <typename E>
__device__ __forceinline__ Chunk<E> find_chunk(const int32_t* __restrict__ prefix, int ntensors,
                                               const E* __restrict__ entries) {
  const int t = find_tensor(prefix, ntensors, blockIdx.x);
  const E e = entries[t];  // read before prefix[t] is needed: one wait covers the entry and the prefix
  const int64_t begin = (int64_t)(blockIdx.x - prefix[t]) * kMTChunk;
  const int64_t end = min(e.numel, begin + (int64_t)kMTChunk);
  return {e, t, begin, end, end - begin == kMTChunk};
}

// Fast path (full chunk, every pointer 16-byte aligned): each thread handles 4 groups of 4 elements strided
// by the block, so that every wave-instruction is a contiguous 1 KiB access. Otherwise element by element.
template <typename E, typename V, typename S>
__device__ __forceinline__ void for_chunk(const Chunk<E>& c, bool aligned, V vec4, S scalar) {
  if (aligned && c.full) {
#pragma unroll
    for (int k = 0; k < kMTPerThread / 4; ++k) vec4(c.begin + ((int64_t)k * kMTBlock + threadIdx.x) * 4);
  } else {
    for (int64_t i = c.begin + threadIdx.x; i < c.end; i += kMTBlock) scalar(i);
  }
}

template <typename... P>
__device__ __forceinline__ bool aligned16(const P*... p) {  // a null pointer counts as aligned
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// 4 consecutive fp32 or bf16 elements (one 16- or 8-byte access), widened to fp32.
template <typename G>
__device__ __forceinline__ float4_t load4_f32(const G* p) {
  if constexpr (sizeof(G) == 4) {
    return *reinterpret_cast<const float4_t*>(p);
  } else {
    const ushort4_t r = *reinterpret_cast<const ushort4_t*>(p);
    return float4_t{bf16_to_f32(r.x), bf16_to_f32(r.y), bf16_to_f32(r.z), bf16_to_f32(r.w)};
  }
}

// --------------------------------------------------------------------------------------------
// SGD with momentum / nesterov / weight decay / dampening; semantics of torch.optim.SGD.
// d = g*grad_scale (+ wd*p); m = first ? d : mu*m + (1-damp)*d; d = nesterov ? d + mu*m : m;
// p -= lr*d. Optionally writes a bf16 shadow copy of the updated parameter.
// --------------------------------------------------------------------------------------------
// kEma: the same pass also advances an fp32 exponential moving average of the updated value,
// ev = fmaf(omd, p_new - ev, ev) with omd = 1 - decay.
template <typename G, bool kMomentum, bool kEma = false>
__device__ __forceinline__ void sgd_body(const Chunk<SgdEntry>& c, const SgdParams& hp, float* ema = nullptr,
                                         float omd = 0.f);

template <typename G, bool kMomentum>
__global__ __launch_bounds__(kMTBlock) void sgd_kernel(const SgdEntry* __restrict__ entries,
                                                       const int32_t* __restrict__ prefix, int ntensors,
                                                       SgdParams hp) {
  sgd_body<G, kMomentum>(find_chunk(prefix, ntensors, entries), hp);
}

// Same update with the tensor list passed BY VALUE in the kernel arguments (no device table): used
// when gradient pointers change every step (autograd-owned gradients, set_to_none zero_grad).
template <typename G, bool kMomentum>
__global__ __launch_bounds__(kMTBlock) void sgd_list_kernel(SgdList list, SgdParams hp) {
  sgd_body<G, kMomentum>(find_chunk(list.prefix, list.ntensors, list.e), hp);
}

// The list kernel with the weight EMA: slot t of `ema` belongs to list.e[t]; omd = 1 - decay is read from
// device memory, so a captured step follows a decay schedule between replays.
template <typename G, bool kMomentum>
__global__ __launch_bounds__(kMTBlock) void sgd_ema_list_kernel(SgdList list, EmaSlots ema,
                                                                const float* __restrict__ omd, SgdParams hp) {
  const auto c = find_chunk(list.prefix, list.ntensors, list.e);
  sgd_body<G, kMomentum, true>(c, hp, ema.ema[c.t], omd[0]);
}

// One chunk of one tensor through `update(p, g, m, p_out, m_out)`: reads p, g (fp32 or bf16) and m,
// writes p, m and the optional bf16 shadow. Shared by the SGD and LARS update kernels. kEma: also reads
// and writes the fp32 average `ev` of the value just stored to p (never of the bf16 shadow).
template <typename G, bool kMomentum, bool kEma = false, typename F>
__device__ __forceinline__ void update_chunk(const Chunk<SgdEntry>& c, F update, float* ema = nullptr,
                                             float omd = 0.f) {
  float* __restrict__ p = c.e.param;
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.grad);
  float* __restrict__ m = c.e.momentum;
  bf16_t* __restrict__ pb = c.e.param_bf16;
  float* __restrict__ ev = ema;
  for_chunk(
      c, aligned16(p, g, kMomentum ? m : nullptr, kEma ? ev : nullptr, pb),
      [&](int64_t i) {
        float4_t pv = *reinterpret_cast<const float4_t*>(p + i);
        float4_t gv = load4_f32(g + i);
        float4_t mv = kMomentum ? *reinterpret_cast<const float4_t*>(m + i) : float4_t{0, 0, 0, 0};
        float4_t ea{0, 0, 0, 0};
        if constexpr (kEma) ea = *reinterpret_cast<const float4_t*>(ev + i);
        float po_[4], mo_[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) update(pv[j], gv[j], mv[j], po_[j], mo_[j]);
        const float4_t po{po_[0], po_[1], po_[2], po_[3]};
        const float4_t mo{mo_[0], mo_[1], mo_[2], mo_[3]};
        *reinterpret_cast<float4_t*>(p + i) = po;
        if (kMomentum) *reinterpret_cast<float4_t*>(m + i) = mo;
        if constexpr (kEma) {
          *reinterpret_cast<float4_t*>(ev + i) = float4_t{fmaf(omd, po.x - ea.x, ea.x), fmaf(omd, po.y - ea.y, ea.y),
                                                          fmaf(omd, po.z - ea.z, ea.z), fmaf(omd, po.w - ea.w, ea.w)};
        }
        if (pb) {
          ushort4_t b{f32_to_bf16(po.x), f32_to_bf16(po.y), f32_to_bf16(po.z), f32_to_bf16(po.w)};
          *reinterpret_cast<ushort4_t*>(pb + i) = b;
        }
      },
      [&](int64_t i) {
        float po, mo = 0.f;
        const float gv = Cvt<G>::to_f32(g[i]);
        update(p[i], gv, kMomentum ? m[i] : 0.f, po, mo);
        p[i] = po;
        if (kMomentum) m[i] = mo;
        if constexpr (kEma) {
          const float ea = ev[i];
          ev[i] = fmaf(omd, po - ea, ea);
        }
        if (pb) pb[i] = f32_to_bf16(po);
      });
}

template <typename G, bool kMomentum, bool kEma>
__device__ __forceinline__ void sgd_body(const Chunk<SgdEntry>& c, const SgdParams& hp, float* ema, float omd) {
  const float lr = hp.lr, mu = hp.momentum, damp1 = 1.f - hp.dampening, wd = hp.weight_decay;
  const float gs = hp.grad_scale;
  const bool first = hp.first_step != 0;
  const bool nest = hp.nesterov != 0;
  update_chunk<G, kMomentum, kEma>(c, [&](float pv, float gv, float mv, float& po, float& mo) {
    float d = gv * gs;
    if (wd != 0.f) d = fmaf(wd, pv, d);
    if (kMomentum) {
      mo = first ? d : fmaf(mu, mv, damp1 * d);
      d = nest ? fmaf(mu, mo, d) : mo;
    }
    po = fmaf(-lr, d, pv);
  }, ema, omd);
}

// --------------------------------------------------------------------------------------------
// EMA of fp32 tensors the optimizer does not step (BatchNorm running statistics), and the in-place
// exchange of fp32 targets with their averages for evaluation. By-value lists like the updates.
// --------------------------------------------------------------------------------------------
// ema = fmaf(omd, target - ema, ema): 8 B/elem read + 4 B/elem written.
__global__ __launch_bounds__(kMTBlock) void ema_update_list_kernel(EmaList list, const float* __restrict__ omd_dev) {
  const auto c = find_chunk(list.prefix, list.ntensors, list.e);
  const float* __restrict__ x = c.e.target;
  float* __restrict__ ev = c.e.ema;
  const float omd = omd_dev[0];
  for_chunk(
      c, aligned16(x, ev),
      [&](int64_t i) {
        const float4_t xv = *reinterpret_cast<const float4_t*>(x + i);
        const float4_t ea = *reinterpret_cast<const float4_t*>(ev + i);
        *reinterpret_cast<float4_t*>(ev + i) = float4_t{fmaf(omd, xv.x - ea.x, ea.x), fmaf(omd, xv.y - ea.y, ea.y),
                                                        fmaf(omd, xv.z - ea.z, ea.z), fmaf(omd, xv.w - ea.w, ea.w)};
      },
      [&](int64_t i) {
        const float ea = ev[i];
        ev[i] = fmaf(omd, x[i] - ea, ea);
      });
}

// target <-> ema; shadow = bf16(new target) where the entry has one. Each element is read and written by one
// thread, so the exchange needs no temporary; a second swap restores every bit (the shadow is a function of
// its master).
__global__ __launch_bounds__(kMTBlock) void ema_swap_list_kernel(EmaList list) {
  const auto c = find_chunk(list.prefix, list.ntensors, list.e);
  float* __restrict__ x = c.e.target;
  float* __restrict__ ev = c.e.ema;
  bf16_t* __restrict__ pb = c.e.shadow;
  for_chunk(
      c, aligned16(x, ev, pb),
      [&](int64_t i) {
        const float4_t xv = *reinterpret_cast<const float4_t*>(x + i);
        const float4_t ea = *reinterpret_cast<const float4_t*>(ev + i);
        *reinterpret_cast<float4_t*>(x + i) = ea;
        *reinterpret_cast<float4_t*>(ev + i) = xv;
        if (pb) {
          ushort4_t b{f32_to_bf16(ea.x), f32_to_bf16(ea.y), f32_to_bf16(ea.z), f32_to_bf16(ea.w)};
          *reinterpret_cast<ushort4_t*>(pb + i) = b;
        }
      },
      [&](int64_t i) {
        const float xv = x[i], ea = ev[i];
        x[i] = ea;
        ev[i] = xv;
        if (pb) pb[i] = f32_to_bf16(ea);
      });
}

// --------------------------------------------------------------------------------------------
// Pack: flat[dst_off : dst_off+n] = (DT)(src * scale)    (tensor fusion, ourdist.py:35)
// Unpack: dst = (DT)(flat[src_off : src_off+n] * scale)  (ourdist.py:42 fused with the 1/N average)
// --------------------------------------------------------------------------------------------
template <typename S, typename D>
__device__ __forceinline__ void copy_scale_range(const S* __restrict__ src, D* __restrict__ dst,
                                                 const Chunk<PackEntry>& c, float scale) {
  for_chunk(
      c, aligned16(src, dst),
      [&](int64_t i) {
        const float4_t v = load4_f32(src + i);
        if constexpr (sizeof(D) == 4) {
          *reinterpret_cast<float4_t*>(reinterpret_cast<float*>(dst) + i) =
              float4_t{v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale};
        } else {
          *reinterpret_cast<ushort4_t*>(reinterpret_cast<bf16_t*>(dst) + i) =
              ushort4_t{f32_to_bf16(v[0] * scale), f32_to_bf16(v[1] * scale), f32_to_bf16(v[2] * scale),
                        f32_to_bf16(v[3] * scale)};
        }
      },
      [&](int64_t i) { dst[i] = Cvt<D>::from_f32(Cvt<S>::to_f32(src[i]) * scale); });
}

template <typename S, typename D>
__global__ __launch_bounds__(kMTBlock) void pack_kernel(const PackEntry* __restrict__ entries,
                                                        const int32_t* __restrict__ prefix, int ntensors,
                                                        void* __restrict__ flat, float scale) {
  const auto c = find_chunk(prefix, ntensors, entries);
  copy_scale_range(reinterpret_cast<const S*>(c.e.tensor), reinterpret_cast<D*>(flat) + c.e.offset, c, scale);
}

template <typename S, typename D>
__global__ __launch_bounds__(kMTBlock) void pack_list_kernel(PackList list, void* __restrict__ flat, float scale) {
  const auto c = find_chunk(list.prefix, list.ntensors, list.e);
  copy_scale_range(reinterpret_cast<const S*>(c.e.tensor), reinterpret_cast<D*>(flat) + c.e.offset, c, scale);
}

template <typename S, typename D>
__global__ __launch_bounds__(kMTBlock) void unpack_kernel(const PackEntry* __restrict__ entries,
                                                          const int32_t* __restrict__ prefix, int ntensors,
                                                          const void* __restrict__ flat, float scale) {
  const auto c = find_chunk(prefix, ntensors, entries);
  copy_scale_range(reinterpret_cast<const S*>(flat) + c.e.offset, reinterpret_cast<D*>(c.e.tensor), c, scale);
}

// ---------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------
void launch_sgd(const SgdEntry* entries, const int32_t* prefix, int ntensors, int nblocks, int grad_dtype,
                bool use_momentum, const SgdParams& hp, hipStream_t stream) {
  if (nblocks <= 0) return;
  dispatch_dtype(grad_dtype, use_momentum, [&](auto g, auto m) {
    hipLaunchKernelGGL((sgd_kernel<tag_t<decltype(g)>, decltype(m)::value>), dim3(nblocks), dim3(kMTBlock), 0, stream,
                       entries, prefix, ntensors, hp);
  });
}

void launch_sgd_list(const SgdList& list, int nblocks, int grad_dtype, bool use_momentum, const SgdParams& hp,
                     hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  dispatch_dtype(grad_dtype, use_momentum, [&](auto g, auto m) {
    hipLaunchKernelGGL((sgd_list_kernel<tag_t<decltype(g)>, decltype(m)::value>), dim3(nblocks), dim3(kMTBlock), 0,
                       stream, list, hp);
  });
}

void launch_sgd_ema_list(const SgdList& list, const EmaSlots& ema, const float* omd, int nblocks, int grad_dtype,
                         bool use_momentum, const SgdParams& hp, hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  dispatch_dtype(grad_dtype, use_momentum, [&](auto g, auto m) {
    hipLaunchKernelGGL((sgd_ema_list_kernel<tag_t<decltype(g)>, decltype(m)::value>), dim3(nblocks), dim3(kMTBlock),
                       0, stream, list, ema, omd, hp);
  });
}

void launch_ema_update_list(const EmaList& list, int nblocks, const float* omd, hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  hipLaunchKernelGGL(ema_update_list_kernel, dim3(nblocks), dim3(kMTBlock), 0, stream, list, omd);
}

void launch_ema_swap_list(const EmaList& list, int nblocks, hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  hipLaunchKernelGGL(ema_swap_list_kernel, dim3(nblocks), dim3(kMTBlock), 0, stream, list);
}

// f(TypeTag<S>, TypeTag<D>) for a (source, destination) dtype pair
template <typename F>
static void dispatch_copy(int src_dtype, int dst_dtype, F f) {
  dispatch_dtype(src_dtype, [&](auto s) { dispatch_dtype(dst_dtype, [&](auto d) { f(s, d); }); });
}

void launch_pack_list(const PackList& list, int nblocks, int src_dtype, int flat_dtype, void* flat, float scale,
                      hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  dispatch_copy(src_dtype, flat_dtype, [&](auto s, auto d) {
    hipLaunchKernelGGL((pack_list_kernel<tag_t<decltype(s)>, tag_t<decltype(d)>>), dim3(nblocks), dim3(kMTBlock), 0,
                       stream, list, flat, scale);
  });
}

void launch_pack(const PackEntry* entries, const int32_t* prefix, int ntensors, int nblocks, int src_dtype,
                 int flat_dtype, void* flat, float scale, hipStream_t stream) {
  if (nblocks <= 0) return;
  dispatch_copy(src_dtype, flat_dtype, [&](auto s, auto d) {
    hipLaunchKernelGGL((pack_kernel<tag_t<decltype(s)>, tag_t<decltype(d)>>), dim3(nblocks), dim3(kMTBlock), 0, stream,
                       entries, prefix, ntensors, flat, scale);
  });
}

void launch_unpack(const PackEntry* entries, const int32_t* prefix, int ntensors, int nblocks, int flat_dtype,
                   int dst_dtype, const void* flat, float scale, hipStream_t stream) {
  if (nblocks <= 0) return;
  dispatch_copy(flat_dtype, dst_dtype, [&](auto s, auto d) {
    hipLaunchKernelGGL((unpack_kernel<tag_t<decltype(s)>, tag_t<decltype(d)>>), dim3(nblocks), dim3(kMTBlock), 0,
                       stream, entries, prefix, ntensors, flat, scale);
  });
}

// --------------------------------------------------------------------------------------------
// Fused LARS (You et al. 2017) and tensor-list L2 norms; layout and formula in dla_kernels.h.
// HBM-bound like SGD: the square-sum pass adds one read of p and g to the update's traffic.
// --------------------------------------------------------------------------------------------
// The block's two sums from every thread's two: the wave butterfly, then the 4 waves through LDS in wave
// order. One plain 8-byte store per block (no atomics: bitwise reproducible).
__device__ __forceinline__ void block_sum2_store(float a, float b, float* out) {
  a = wave_sum(a);
  b = wave_sum(b);
  __shared__ float sm[2][kMTBlock / kWave];
  const int wave = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
    sm[0][wave] = a;
    sm[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sm[0][0];
    b = sm[1][0];
#pragma unroll
    for (int w = 1; w < kMTBlock / kWave; ++w) {
      a += sm[0][w];
      b += sm[1][w];
    }
    out[0] = a;
    out[1] = b;
  }
}

// Square sums of one chunk: 16 elements per thread accumulated in fp32 in a fixed order, then
// block_sum2_store.
template <typename G>
__global__ __launch_bounds__(kMTBlock) void sqsum_list_kernel(LarsList list, float* __restrict__ partials) {
  const auto c = find_chunk(list.l.prefix, list.l.ntensors, list.l.e);
  const float* __restrict__ p = c.e.param;
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.grad);
  float sp = 0.f, sg = 0.f;
  for_chunk(
      c, aligned16(p, g),
      [&](int64_t i) {
        const float4_t gv = load4_f32(g + i);
        const float4_t pv = p ? *reinterpret_cast<const float4_t*>(p + i) : float4_t{0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sg = fmaf(gv[j], gv[j], sg);
          sp = fmaf(pv[j], pv[j], sp);
        }
      },
      [&](int64_t i) {
        const float gv = Cvt<G>::to_f32(g[i]);
        sg = fmaf(gv, gv, sg);
        if (p) sp = fmaf(p[i], p[i], sp);
      });
  block_sum2_store(sp, sg, partials + 2 * ((int64_t)list.block_base + blockIdx.x));
}

// One block of 16 waves. Wave w sums the partial ranges of tensors w, w + 16, ... (lane-strided, then
// the wave butterfly: a fixed order) and keeps their squared sums in the norms slots; the waves'
// gradient totals meet in LDS. Then every thread turns squared sums into norms, trust ratios and
// local rates. The block is latency-bound (a table row, then its partials, per tensor), so it has 16
// waves and fetches the next row ahead: on ResNet-50's 161 tensors a 4-wave block without the
// prefetch took 42 us, a third of the whole SGD step (both forms timed in profiles/lars/README.md).
constexpr int kFinBlock = 1024;
constexpr int kFinWaves = kFinBlock / kWave;

__global__ __launch_bounds__(kFinBlock) void lars_finalize_kernel(const LarsTensor* __restrict__ table, int ntensors,
                                                                  const float* __restrict__ lr_dev, float grad_scale,
                                                                  float max_grad_norm, float* ws) {
  float* local_lr = ws + kLarsHead;
  float* norms = local_lr + ntensors;
  const float2* partials = reinterpret_cast<const float2*>(ws + lars_partials_offset(ntensors));
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float total = 0.f;
  int nb = 0, ne = 0;
  if (wave < ntensors) {
    nb = table[wave].part_begin;
    ne = table[wave].part_end;
  }
  for (int t = wave; t < ntensors; t += kFinWaves) {
    const int b = nb, e = ne;
    if (t + kFinWaves < ntensors) {
      nb = table[t + kFinWaves].part_begin;
      ne = table[t + kFinWaves].part_end;
    }
    float sp = 0.f, sg = 0.f;
    for (int i = b + lane; i < e; i += kWave) {
      const float2 v = partials[i];
      sp += v.x;
      sg += v.y;
    }
    sp = wave_sum(sp);
    sg = wave_sum(sg);
    total += sg;
    if (lane == 0) {
      norms[2 * t] = sp;
      norms[2 * t + 1] = sg;
    }
  }
  __shared__ float sm[kFinWaves];
  if (lane == 0) sm[wave] = total;
  __syncthreads();  // also orders the squared sums stored above before the loads below
  total = sm[0];
#pragma unroll
  for (int w = 1; w < kFinWaves; ++w) total += sm[w];
  const float gnorm = grad_scale * sqrtf(total);
  const float clip = max_grad_norm > 0.f ? fminf(1.f, max_grad_norm / (gnorm + 1e-6f)) : 1.f;
  const float c = grad_scale * clip;
  if (threadIdx.x == 0) {
    ws[0] = c;
    ws[1] = gnorm;
    ws[2] = clip;
    ws[3] = 0.f;
  }
  for (int t = threadIdx.x; t < ntensors; t += kFinBlock) {
    const LarsTensor r = table[t];
    const float wn = sqrtf(norms[2 * t]), gr = sqrtf(norms[2 * t + 1]);
    const float gn = c * gr;
    float trust = 1.f;
    if (r.adapt && wn > 0.f && gn > 0.f) trust = r.eta * wn / (gn + r.weight_decay * wn + r.eps);
    local_lr[t] = lr_dev ? lr_dev[r.group] * trust : trust;
    norms[2 * t] = wn;
    norms[2 * t + 1] = gr;
  }
}

template <typename G, bool kEma>
__device__ __forceinline__ void lars_body(const LarsList& list, const LarsTensor* __restrict__ table,
                                          const float* __restrict__ ws, const Chunk<SgdEntry>& ch, float* ema,
                                          float omd) {
  const int row = list.tensor_base + ch.t;
  const float c = ws[0], llr = ws[kLarsHead + row];
  const float wd = table[row].weight_decay, mu = table[row].momentum;
  update_chunk<G, true, kEma>(ch, [&](float pv, float gv, float mv, float& po, float& mo) {
    float d = gv * c;
    if (wd != 0.f) d = fmaf(wd, pv, d);
    mo = fmaf(mu, mv, llr * d);
    po = pv - mo;
  }, ema, omd);
}

template <typename G>
__global__ __launch_bounds__(kMTBlock) void lars_list_kernel(LarsList list, const LarsTensor* __restrict__ table,
                                                             const float* __restrict__ ws) {
  lars_body<G, false>(list, table, ws, find_chunk(list.l.prefix, list.l.ntensors, list.l.e), nullptr, 0.f);
}

template <typename G>
__global__ __launch_bounds__(kMTBlock) void lars_ema_list_kernel(LarsList list, EmaSlots ema,
                                                                 const float* __restrict__ omd,
                                                                 const LarsTensor* __restrict__ table,
                                                                 const float* __restrict__ ws) {
  const auto c = find_chunk(list.l.prefix, list.l.ntensors, list.l.e);
  lars_body<G, true>(list, table, ws, c, ema.ema[c.t], omd[0]);
}

void launch_sqsum_list(const LarsList& list, int nblocks, int grad_dtype, float* ws, int ntensors,
                       hipStream_t stream) {
  if (nblocks <= 0 || list.l.ntensors <= 0) return;
  float* partials = ws + lars_partials_offset(ntensors);
  dispatch_dtype(grad_dtype, [&](auto g) {
    hipLaunchKernelGGL((sqsum_list_kernel<tag_t<decltype(g)>>), dim3(nblocks), dim3(kMTBlock), 0, stream, list,
                       partials);
  });
}

void launch_lars_finalize(const LarsTensor* table, int ntensors, const float* lr_dev, float grad_scale,
                          float max_grad_norm, float* ws, hipStream_t stream) {
  if (ntensors <= 0) return;
  hipLaunchKernelGGL(lars_finalize_kernel, dim3(1), dim3(kFinBlock), 0, stream, table, ntensors, lr_dev, grad_scale,
                     max_grad_norm, ws);
}

void launch_lars_list(const LarsList& list, int nblocks, int grad_dtype, const LarsTensor* table, const float* ws,
                      hipStream_t stream) {
  if (nblocks <= 0 || list.l.ntensors <= 0) return;
  dispatch_dtype(grad_dtype, [&](auto g) {
    hipLaunchKernelGGL((lars_list_kernel<tag_t<decltype(g)>>), dim3(nblocks), dim3(kMTBlock), 0, stream, list, table,
                       ws);
  });
}

void launch_lars_ema_list(const LarsList& list, const EmaSlots& ema, const float* omd, int nblocks, int grad_dtype,
                          const LarsTensor* table, const float* ws, hipStream_t stream) {
  if (nblocks <= 0 || list.l.ntensors <= 0) return;
  dispatch_dtype(grad_dtype, [&](auto g) {
    hipLaunchKernelGGL((lars_ema_list_kernel<tag_t<decltype(g)>>), dim3(nblocks), dim3(kMTBlock), 0, stream, list, ema,
                       omd, table, ws);
  });
}

// --------------------------------------------------------------------------------------------
// Fused LAMB (You et al. 2019) and AdamW; passes, formula and layouts in dla_kernels.h. HBM-bound:
// with bf16 gradients and shadows the LAMB moments pass moves 22 B/elem, its apply pass 18, the
// one-pass AdamW update 28 (+ 8 each for the weight EMA). Times: profiles/lamb/README.md.
// --------------------------------------------------------------------------------------------
struct AdamCoef {
  float c;                   // grad_scale * clip
  float b1, omb1, b2, omb2;  // beta, 1 - beta
  float bc1, bc2;            // 1 - beta^k
  float eps, wd, alpha;      // alpha = lr * trust
};

// 1 - beta^k from ln(beta): relative error ~1e-7 for every k, where a running fp32 product beta^k drifts.
__device__ __forceinline__ float bias_correction(int k, float ln_beta) {
  return -expm1f(__fmul_rn((float)k, ln_beta));
}

__device__ __forceinline__ AdamCoef adam_coef(const AdamTensor& r, float c, float bc1, float bc2, float alpha) {
  return {c, r.beta1, r.omb1, r.beta2, r.omb2, bc1, bc2, r.eps, r.weight_decay, alpha};
}

// One element. kGrad: the gradient enters the moments; kApply: the parameter is stepped, otherwise p^2 and
// u^2 are accumulated. Both LAMB passes and the AdamW pass form u by this one expression (plain divisions
// and square root: the bound of the tests leaves no room for the approximate forms).
template <bool kGrad, bool kApply>
__device__ __forceinline__ void adam_elem(const AdamCoef& h, float& p, float g, float& m, float& v, float& sp,
                                          float& su) {
  if constexpr (kGrad) {
    const float gh = h.c * g;
    m = fmaf(h.b1, m, h.omb1 * gh);
    v = fmaf(h.b2, v, (h.omb2 * gh) * gh);
  }
  const float u = fmaf(h.wd, p, (m / h.bc1) / (sqrtf(v / h.bc2) + h.eps));
  if constexpr (kApply) {
    p = fmaf(-h.alpha, u, p);
  } else {
    sp = fmaf(p, p, sp);
    su = fmaf(u, u, su);
  }
}

// update_chunk's sibling for two moment buffers. Reads p, m, v and with kGrad g (fp32 or bf16); writes m, v
// with kGrad, and p, the optional bf16 shadow and with kEma the average with kApply.
template <typename G, bool kGrad, bool kApply, bool kEma>
__device__ __forceinline__ void adam_chunk(const Chunk<AdamEntry>& c, const AdamCoef& h, float* ema, float omd,
                                           float& sp, float& su) {
  static_assert(kApply || !kEma, "the average follows the stored parameter");
  float* __restrict__ p = c.e.param;
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.grad);
  float* __restrict__ m = c.e.m;
  float* __restrict__ v = c.e.v;
  bf16_t* __restrict__ pb = kApply ? c.e.param_bf16 : nullptr;
  float* __restrict__ ev = ema;
  for_chunk(
      c, aligned16(p, kGrad ? g : nullptr, m, v, kEma ? ev : nullptr, pb),
      [&](int64_t i) {
        const float4_t pv = *reinterpret_cast<const float4_t*>(p + i);
        float4_t gv{0, 0, 0, 0};
        if constexpr (kGrad) gv = load4_f32(g + i);
        const float4_t mv = *reinterpret_cast<const float4_t*>(m + i);
        const float4_t vv = *reinterpret_cast<const float4_t*>(v + i);
        float4_t ea{0, 0, 0, 0};
        if constexpr (kEma) ea = *reinterpret_cast<const float4_t*>(ev + i);
        float po[4] = {pv.x, pv.y, pv.z, pv.w}, mo[4] = {mv.x, mv.y, mv.z, mv.w}, vo[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) adam_elem<kGrad, kApply>(h, po[j], gv[j], mo[j], vo[j], sp, su);
        if constexpr (kGrad) {
          *reinterpret_cast<float4_t*>(m + i) = float4_t{mo[0], mo[1], mo[2], mo[3]};
          *reinterpret_cast<float4_t*>(v + i) = float4_t{vo[0], vo[1], vo[2], vo[3]};
        }
        if constexpr (kApply) {
          *reinterpret_cast<float4_t*>(p + i) = float4_t{po[0], po[1], po[2], po[3]};
          if constexpr (kEma) {
            *reinterpret_cast<float4_t*>(ev + i) =
                float4_t{fmaf(omd, po[0] - ea.x, ea.x), fmaf(omd, po[1] - ea.y, ea.y), fmaf(omd, po[2] - ea.z, ea.z),
                         fmaf(omd, po[3] - ea.w, ea.w)};
          }
          if (pb) {
            *reinterpret_cast<ushort4_t*>(pb + i) =
                ushort4_t{f32_to_bf16(po[0]), f32_to_bf16(po[1]), f32_to_bf16(po[2]), f32_to_bf16(po[3])};
          }
        }
      },
      [&](int64_t i) {
        float po = p[i], mo = m[i], vo = v[i], gv = 0.f;
        if constexpr (kGrad) gv = Cvt<G>::to_f32(g[i]);
        adam_elem<kGrad, kApply>(h, po, gv, mo, vo, sp, su);
        if constexpr (kGrad) {
          m[i] = mo;
          v[i] = vo;
        }
        if constexpr (kApply) {
          p[i] = po;
          if constexpr (kEma) {
            const float ea = ev[i];
            ev[i] = fmaf(omd, po - ea, ea);
          }
          if (pb) pb[i] = f32_to_bf16(po);
        }
      });
}

// LAMB pass 1: the moments, and this block's (sum p^2, sum u^2) with u formed in registers and never stored.
// The finalize has not committed this step's count yet, so k = step + 1.
template <typename G>
__global__ __launch_bounds__(kMTBlock) void lamb_moments_list_kernel(AdamList list, int tensor_base, int block_base,
                                                                     const AdamTensor* __restrict__ table,
                                                                     const float* __restrict__ ws_clip,
                                                                     float grad_scale, float* __restrict__ partials) {
  const auto ch = find_chunk(list.prefix, list.ntensors, list.e);
  const AdamTensor r = table[tensor_base + ch.t];
  const int k = r.step[0] + 1;
  const AdamCoef h = adam_coef(r, ws_clip ? ws_clip[0] : grad_scale, bias_correction(k, r.ln_beta1),
                               bias_correction(k, r.ln_beta2), 0.f);
  float sp = 0.f, su = 0.f;
  adam_chunk<G, true, false, false>(ch, h, nullptr, 0.f, sp, su);
  block_sum2_store(sp, su, partials + 2 * ((int64_t)block_base + blockIdx.x));
}

// One block, the shape of lars_finalize_kernel (16 waves, the next table row fetched ahead). trust: wave w
// sums the (p^2, u^2) partials of tensors w, w + 16, ...; grad_partials: the same walk over the (., g^2)
// partials of a gradient square-sum pass in ws_clip, whose total gives G, clip and c as in LARS. Then every
// thread forms its tensors' bias corrections, trust and alpha, and commits step + 1.
__global__ __launch_bounds__(kFinBlock) void adam_finalize_kernel(const AdamTensor* __restrict__ table, int ntensors,
                                                                  const float* __restrict__ lr_dev, int trust,
                                                                  int grad_partials, float grad_scale,
                                                                  float max_grad_norm, float* ws_clip, float* ws) {
  float* alpha = ws;
  float* bc = ws + ntensors;
  float* norms = ws + 3 * (int64_t)ntensors;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (trust || grad_partials) {  // uniform over the block
    const float2* partials = reinterpret_cast<const float2*>(
        trust ? ws + adam_partials_offset(ntensors) : ws_clip + lars_partials_offset(ntensors));
    float total = 0.f;
    int nb = 0, ne = 0;
    if (wave < ntensors) {
      nb = table[wave].part_begin;
      ne = table[wave].part_end;
    }
    for (int t = wave; t < ntensors; t += kFinWaves) {
      const int b = nb, e = ne;
      if (t + kFinWaves < ntensors) {
        nb = table[t + kFinWaves].part_begin;
        ne = table[t + kFinWaves].part_end;
      }
      float sa = 0.f, sb = 0.f;
      for (int i = b + lane; i < e; i += kWave) {
        const float2 v = partials[i];
        sa += v.x;
        sb += v.y;
      }
      sa = wave_sum(sa);
      sb = wave_sum(sb);
      total += sb;
      if (trust && lane == 0) {
        norms[2 * t] = sa;
        norms[2 * t + 1] = sb;
      }
    }
    __shared__ float sm[kFinWaves];
    if (lane == 0) sm[wave] = total;
    __syncthreads();  // also orders the squared sums stored above before the loads below
    if (grad_partials && threadIdx.x == 0) {
      total = sm[0];
#pragma unroll
      for (int w = 1; w < kFinWaves; ++w) total += sm[w];
      const float gnorm = grad_scale * sqrtf(total);
      const float clip = max_grad_norm > 0.f ? fminf(1.f, max_grad_norm / (gnorm + 1e-6f)) : 1.f;
      ws_clip[0] = grad_scale * clip;
      ws_clip[1] = gnorm;
      ws_clip[2] = clip;
      ws_clip[3] = 0.f;
    }
  }
  for (int t = threadIdx.x; t < ntensors; t += kFinBlock) {
    const AdamTensor r = table[t];
    const int k = r.step[0] + 1;
    float tr = 1.f;
    if (trust) {
      const float wn = sqrtf(norms[2 * t]), un = sqrtf(norms[2 * t + 1]);
      if (r.adapt && wn > 0.f && un > 0.f) tr = wn / un;
      norms[2 * t] = wn;
      norms[2 * t + 1] = un;
    }
    alpha[t] = lr_dev[r.group] * tr;
    bc[2 * t] = bias_correction(k, r.ln_beta1);
    bc[2 * t + 1] = bias_correction(k, r.ln_beta2);
    r.step[0] = k;
  }
}

// What the passes after the finalize read of it: table row, alpha and the bias corrections of row `row`.
__device__ __forceinline__ AdamCoef adam_coef_final(const AdamTensor* __restrict__ table, const float* __restrict__ ws,
                                                    int ntensors, int row, float c) {
  return adam_coef(table[row], c, ws[ntensors + 2 * row], ws[ntensors + 2 * row + 1], ws[row]);
}

// LAMB pass 3: u again from p, m, v (no gradient read, no u buffer), p -= alpha u.
template <bool kEma>
__device__ __forceinline__ void lamb_apply_body(const Chunk<AdamEntry>& ch, int row, const AdamTensor* table,
                                                const float* ws, int ntensors, float* ema, float omd) {
  float sp = 0.f, su = 0.f;  // unused: kApply
  adam_chunk<float, false, true, kEma>(ch, adam_coef_final(table, ws, ntensors, row, 0.f), ema, omd, sp, su);
}

__global__ __launch_bounds__(kMTBlock) void lamb_apply_list_kernel(AdamList list, int tensor_base,
                                                                   const AdamTensor* __restrict__ table,
                                                                   const float* __restrict__ ws, int ntensors) {
  const auto ch = find_chunk(list.prefix, list.ntensors, list.e);
  lamb_apply_body<false>(ch, tensor_base + ch.t, table, ws, ntensors, nullptr, 0.f);
}

__global__ __launch_bounds__(kMTBlock) void lamb_apply_ema_list_kernel(AdamList list, int tensor_base, EmaSlots ema,
                                                                       const float* __restrict__ omd,
                                                                       const AdamTensor* __restrict__ table,
                                                                       const float* __restrict__ ws, int ntensors) {
  const auto ch = find_chunk(list.prefix, list.ntensors, list.e);
  lamb_apply_body<true>(ch, tensor_base + ch.t, table, ws, ntensors, ema.ema[ch.t], omd[0]);
}

// AdamW: moments and update in one pass, after the finalize (alpha = lr, no norm work).
template <typename G, bool kEma>
__device__ __forceinline__ void adamw_body(const Chunk<AdamEntry>& ch, int row, const AdamTensor* table,
                                           const float* ws_clip, float grad_scale, const float* ws, int ntensors,
                                           float* ema, float omd) {
  float sp = 0.f, su = 0.f;  // unused: kApply
  adam_chunk<G, true, true, kEma>(
      ch, adam_coef_final(table, ws, ntensors, row, ws_clip ? ws_clip[0] : grad_scale), ema, omd, sp, su);
}

template <typename G>
__global__ __launch_bounds__(kMTBlock) void adamw_list_kernel(AdamList list, int tensor_base,
                                                              const AdamTensor* __restrict__ table,
                                                              const float* __restrict__ ws_clip, float grad_scale,
                                                              const float* __restrict__ ws, int ntensors) {
  const auto ch = find_chunk(list.prefix, list.ntensors, list.e);
  adamw_body<G, false>(ch, tensor_base + ch.t, table, ws_clip, grad_scale, ws, ntensors, nullptr, 0.f);
}

template <typename G>
__global__ __launch_bounds__(kMTBlock) void adamw_ema_list_kernel(AdamList list, int tensor_base, EmaSlots ema,
                                                                  const float* __restrict__ omd,
                                                                  const AdamTensor* __restrict__ table,
                                                                  const float* __restrict__ ws_clip, float grad_scale,
                                                                  const float* __restrict__ ws, int ntensors) {
  const auto ch = find_chunk(list.prefix, list.ntensors, list.e);
  adamw_body<G, true>(ch, tensor_base + ch.t, table, ws_clip, grad_scale, ws, ntensors, ema.ema[ch.t], omd[0]);
}

void launch_lamb_moments_list(const AdamList& list, int tensor_base, int block_base, int nblocks, int grad_dtype,
                              const AdamTensor* table, const float* ws_clip, float grad_scale, float* ws, int ntensors,
                              hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  float* partials = ws + adam_partials_offset(ntensors);
  dispatch_dtype(grad_dtype, [&](auto g) {
    hipLaunchKernelGGL((lamb_moments_list_kernel<tag_t<decltype(g)>>), dim3(nblocks), dim3(kMTBlock), 0, stream, list,
                       tensor_base, block_base, table, ws_clip, grad_scale, partials);
  });
}

void launch_adam_finalize(const AdamTensor* table, int ntensors, const float* lr_dev, bool trust, bool grad_partials,
                          float grad_scale, float max_grad_norm, float* ws_clip, float* ws, hipStream_t stream) {
  if (ntensors <= 0) return;
  hipLaunchKernelGGL(adam_finalize_kernel, dim3(1), dim3(kFinBlock), 0, stream, table, ntensors, lr_dev, trust ? 1 : 0,
                     grad_partials ? 1 : 0, grad_scale, max_grad_norm, ws_clip, ws);
}

void launch_lamb_apply_list(const AdamList& list, int tensor_base, int nblocks, const EmaSlots* ema, const float* omd,
                            const AdamTensor* table, const float* ws, int ntensors, hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  if (ema) {
    hipLaunchKernelGGL(lamb_apply_ema_list_kernel, dim3(nblocks), dim3(kMTBlock), 0, stream, list, tensor_base, *ema,
                       omd, table, ws, ntensors);
  } else {
    hipLaunchKernelGGL(lamb_apply_list_kernel, dim3(nblocks), dim3(kMTBlock), 0, stream, list, tensor_base, table, ws,
                       ntensors);
  }
}

void launch_adamw_list(const AdamList& list, int tensor_base, int nblocks, int grad_dtype, const EmaSlots* ema,
                       const float* omd, const AdamTensor* table, const float* ws_clip, float grad_scale,
                       const float* ws, int ntensors, hipStream_t stream) {
  if (nblocks <= 0 || list.ntensors <= 0) return;
  dispatch_dtype(grad_dtype, [&](auto g) {
    using G = tag_t<decltype(g)>;
    if (ema) {
      hipLaunchKernelGGL((adamw_ema_list_kernel<G>), dim3(nblocks), dim3(kMTBlock), 0, stream, list, tensor_base, *ema,
                         omd, table, ws_clip, grad_scale, ws, ntensors);
    } else {
      hipLaunchKernelGGL((adamw_list_kernel<G>), dim3(nblocks), dim3(kMTBlock), 0, stream, list, tensor_base, table,
                         ws_clip, grad_scale, ws, ntensors);
    }
  });
}

}  // namespace dla
