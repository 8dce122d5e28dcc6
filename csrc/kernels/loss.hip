// Fused log-softmax + NLL loss (mean reduction, ignore_index < 0) forward and backward.
//
// Replaces the two-op chain `F.log_softmax(x)` -> `F.nll_loss(out, target)`
// (/root/reference/src/network.py:29,41 and /root/reference/src/main.py:76), which materialises
// the [B, C] log-probabilities in fp32 and reads them again in backward. Here one wave owns one
// row: max and sum-of-exp are wave reductions (64-lane shuffles), only the row's logsumexp is
// kept (4 B/row) and backward recomputes softmax from the logits.
// The batch mean is summed by a single workgroup in a fixed order, so the loss is bitwise
// reproducible run to run (no float atomics).
#include "dla_common.h"
#include "dla_kernels.h"

namespace dla {

constexpr int kXWaves = 4;

template <typename T>
__global__ __launch_bounds__(kXWaves * 64) void xent_rows_kernel(const T* __restrict__ logits,
                                                                 const int64_t* __restrict__ target,
                                                                 float* __restrict__ ws, int B, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (int64_t)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, Cvt<T>::to_f32(x[c]));
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(Cvt<T>::to_f32(x[c]) - m);
  s = wave_sum(s);
  if (lane == 0) {
    const float lse = m + __logf(s);
    const int64_t t = target[row];
    const bool valid = t >= 0 && t < C;
    ws[row] = lse;
    ws[B + row] = valid ? lse - Cvt<T>::to_f32(x[t]) : 0.f;
    ws[2 * B + row] = valid ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(256) void xent_mean_kernel(const float* __restrict__ ws, float* __restrict__ loss_out,
                                                        int B) {
  __shared__ float red[2][4];
  float s = 0.f, cnt = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) {
    s += ws[B + i];
    cnt += ws[2 * B + i];
  }
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float ts = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const float tc = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    loss_out[0] = tc > 0.f ? ts / tc : NAN;
    loss_out[1] = tc;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                       const float* __restrict__ ws, const float* __restrict__ loss_out,
                                                       const float* __restrict__ gout, T* __restrict__ dlogits, int B,
                                                       int C) {
  const int64_t total = (int64_t)B * C;
  const float g = gout[0] / loss_out[1];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int row = (int)(i / C);
    const int c = (int)(i - (int64_t)row * C);
    const int64_t t = target[row];
    const bool valid = t >= 0 && t < C;
    float d = 0.f;
    if (valid) d = (__expf(Cvt<T>::to_f32(logits[i]) - ws[row]) - (c == t ? 1.f : 0.f)) * g;
    dlogits[i] = Cvt<T>::from_f32(d);
  }
}

void launch_xent_fwd(const void* logits, const int64_t* target, float* ws, float* loss_out, int B, int C, int dtype,
                     hipStream_t stream) {
  dim3 grid((B + kXWaves - 1) / kXWaves), block(kXWaves * 64);
  dispatch_dtype(dtype, [&](auto t) {
    using T = tag_t<decltype(t)>;
    hipLaunchKernelGGL(xent_rows_kernel<T>, grid, block, 0, stream, (const T*)logits, target, ws, B, C);
  });
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(256), 0, stream, ws, loss_out, B);
}

void launch_xent_bwd(const void* logits, const int64_t* target, const float* ws, const float* loss_out,
                     const float* gout, void* dlogits, int B, int C, int dtype, hipStream_t stream) {
  const int64_t total = (int64_t)B * C;
  int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
  dispatch_dtype(dtype, [&](auto t) {
    using T = tag_t<decltype(t)>;
    hipLaunchKernelGGL(xent_bwd_kernel<T>, dim3(grid), dim3(256), 0, stream, (const T*)logits, target, ws, loss_out,
                       gout, (T*)dlogits, B, C);
  });
}

// ------------------------------------------------------------------------------------------------
// Label-smoothed cross-entropy with top-1 / top-k counts (the second forward/backward pair).
//
// Forward rows kernel: one wave per row, each logit loaded once. A lane keeps a running max and a
// sum rescaled to it (online softmax), the plain sum of its logits (the smoothing term) and how many
// of its logits outrank the target's; the lanes are merged at the end. The target's logit is read
// first (one wave-uniform load), so the rank needs no second pass.
// Rows whose base address and pitch are multiples of 16 bytes move 16 bytes per lane per access;
// any other layout takes the scalar path.
// Forward batch kernel: one workgroup, fixed order, no float atomics, like xent_mean_kernel.
// Backward: one wave per row, row constants (target, lse, gout / count) read once per row.
// ------------------------------------------------------------------------------------------------
template <typename T> struct Raw16;  // one 16-byte access: 8 bf16 or 4 fp32
template <> struct Raw16<bf16_t> {
  static constexpr int kN = 8;
  ushort8_t v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const ushort8_t*>(p); }
  __device__ __forceinline__ void store(bf16_t* p) const { *reinterpret_cast<ushort8_t*>(p) = v; }
  __device__ __forceinline__ float get(int j) const { return bf16_to_f32(v[j]); }
  __device__ __forceinline__ void set(int j, float f) { v[j] = f32_to_bf16(f); }
};
template <> struct Raw16<float> {
  static constexpr int kN = 4;
  float4_t v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4_t*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4_t*>(p) = v; }
  __device__ __forceinline__ float get(int j) const { return v[j]; }
  __device__ __forceinline__ void set(int j, float f) { v[j] = f; }
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// Running (max m, sum s of exp(x - m)) of one lane. A lane that has seen nothing, or only -inf, holds
// m = -inf and s = 0: nothing is rescaled from m = -inf and a -inf logit adds exactly 0, so
// exp(-inf - (-inf)) is never formed. A NaN logit still reaches s.
struct OnlineLse {
  float m = -INFINITY, s = 0.f;
  __device__ __forceinline__ void rescale(float mn) {
    if (m != -INFINITY) s *= __expf(m - mn);
    m = mn;
  }
  __device__ __forceinline__ void add(float x) {  // after rescale() to a max that covers x
    s += x == -INFINITY ? 0.f : __expf(x - m);
  }
};

// What one lane knows about its part of the row.
struct RowAcc {
  OnlineLse o;
  float sum = 0.f;  // plain sum of the logits, for the smoothing term
  int above = 0;    // logits that outrank the target: larger, or equal with a smaller class index
  __device__ __forceinline__ void count(float x, int c, float xt, int t) { above += (x > xt) || (x == xt && c < t); }
};

constexpr int kXUnroll = 4;  // 16-byte loads in flight per lane

template <typename T, bool kVec>
__global__ __launch_bounds__(kXWaves * 64) void xent_metric_rows_kernel(const T* __restrict__ logits,
                                                                        const int64_t* __restrict__ target,
                                                                        float* __restrict__ ws, int B, int C,
                                                                        float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (int64_t)row * C;
  const int64_t t64 = target[row];
  const bool valid = t64 >= 0 && t64 < C;
  const int t = valid ? (int)t64 : 0;
  const float xt = Cvt<T>::to_f32(x[t]);  // C >= 1: column 0 exists also for an ignored row
  RowAcc a;
  if constexpr (kVec) {
    constexpr int N = Raw16<T>::kN;
    const int nvec = C / N;  // exact: the pitch is a multiple of 16 bytes
    for (int v0 = lane; v0 < nvec; v0 += 64 * kXUnroll) {
      Raw16<T> r[kXUnroll];
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u)
        if (v0 + 64 * u < nvec) r[u].load(x + (int64_t)(v0 + 64 * u) * N);
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u) {
        if (v0 + 64 * u >= nvec) break;
        float f[N];
        float vm = -INFINITY;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          f[j] = r[u].get(j);
          vm = fmaxf(vm, f[j]);
        }
        a.o.rescale(fmaxf(a.o.m, vm));
#pragma unroll
        for (int j = 0; j < N; ++j) {
          a.o.add(f[j]);
          a.sum += f[j];
          a.count(f[j], (v0 + 64 * u) * N + j, xt, t);
        }
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float f = Cvt<T>::to_f32(x[c]);
      a.o.rescale(fmaxf(a.o.m, f));
      a.o.add(f);
      a.sum += f;
      a.count(f, c, xt, t);
    }
  }
  const float m = wave_max(a.o.m);
  a.o.rescale(m);  // a lane still at -inf keeps its s (0, or NaN from a NaN logit)
  const float s = wave_sum(a.o.s);
  const float sum = wave_sum(a.sum);
  const int above = wave_sum_int(a.above);
  if (lane == 0) {
    const float lse = m + __logf(s);
    // eps == 0 leaves the sum out (as the plain loss does), so a -inf logit does not turn 0 * inf into NaN
    const float smooth = eps > 0.f ? eps * (sum / (float)C) : 0.f;
    ws[row] = lse;
    ws[B + row] = valid ? lse - (1.f - eps) * xt - smooth : 0.f;
    ws[2 * B + row] = valid ? 1.f : 0.f;
    // rank of the target; +inf (never below any k) for an ignored row or a NaN target logit
    ws[3 * B + row] = (valid && xt == xt) ? (float)above : INFINITY;
  }
}

// stats = [sum of row losses over valid rows, valid rows, rows with rank < 1, rows with rank < k];
// ws[4 * B] = stats[0] / stats[1], the mean loss (NaN without a valid row)
__global__ __launch_bounds__(256) void xent_stats_kernel(float* __restrict__ ws, float* __restrict__ stats, int B,
                                                         int k) {
  __shared__ float red[4][4];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float kf = (float)k;
  for (int i = threadIdx.x; i < B; i += 256) {
    const float rank = ws[3 * B + i];
    acc[0] += ws[B + i];
    acc[1] += ws[2 * B + i];
    acc[2] += rank < 1.f ? 1.f : 0.f;
    acc[3] += rank < kf ? 1.f : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] = wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      tot[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
      stats[q] = tot[q];
    }
    ws[4 * B] = tot[1] > 0.f ? tot[0] / tot[1] : NAN;
  }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(kXWaves * 64) void xent_smooth_bwd_kernel(const T* __restrict__ logits,
                                                                       const int64_t* __restrict__ target,
                                                                       const float* __restrict__ ws,
                                                                       const float* __restrict__ stats,
                                                                       const float* __restrict__ gout,
                                                                       T* __restrict__ dlogits, int B, int C,
                                                                       float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (int64_t)row * C;
  T* d = dlogits + (int64_t)row * C;
  const int64_t t64 = target[row];
  const bool valid = t64 >= 0 && t64 < C;
  const int t = valid ? (int)t64 : -1;
  const float lse = ws[row];
  const float g = valid ? gout[0] / stats[1] : 0.f;  // one division per row
  const float hot = 1.f - eps, uni = eps / (float)C;
  if constexpr (kVec) {
    constexpr int N = Raw16<T>::kN;
    const int nvec = C / N;
    for (int v0 = lane; v0 < nvec; v0 += 64 * kXUnroll) {
      Raw16<T> r[kXUnroll];
      if (valid) {
#pragma unroll
        for (int u = 0; u < kXUnroll; ++u)
          if (v0 + 64 * u < nvec) r[u].load(x + (int64_t)(v0 + 64 * u) * N);
      }
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u) {
        if (v0 + 64 * u >= nvec) break;
        const int c0 = (v0 + 64 * u) * N;
        Raw16<T> o;
#pragma unroll
        for (int j = 0; j < N; ++j)
          o.set(j, valid ? (__expf(r[u].get(j) - lse) - (c0 + j == t ? hot : 0.f) - uni) * g : 0.f);
        o.store(d + c0);
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float v = 0.f;
      if (valid) v = (__expf(Cvt<T>::to_f32(x[c]) - lse) - (c == t ? hot : 0.f) - uni) * g;
      d[c] = Cvt<T>::from_f32(v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Pair-target (Mixup / CutMix) label-smoothed cross-entropy: row targets (ta, tb) with weights
// (lam, 1 - lam). The same row kernels as above without the rank: both target logits are read first
// (two wave-uniform loads), then every logit is loaded once in forward and once in backward.
//   xt  = lam * x[ta] + (1 - lam) * x[tb]      (a term whose weight is exactly 0 is left out)
//   row = lse - (1 - eps) * xt - (eps > 0 ? eps * mean(x) : 0)
// A row is valid iff both targets are in [0, C). With lam == 1 (or 0) every operation on the row is
// the one xent_metric_rows_kernel / xent_smooth_bwd_kernel does for ta (tb), in the same order.
// ------------------------------------------------------------------------------------------------
struct MixRowAcc {
  OnlineLse o;
  float sum = 0.f;  // plain sum of the logits, for the smoothing term
};

template <typename T, bool kVec>
__global__ __launch_bounds__(kXWaves * 64) void xent_mix_rows_kernel(const T* __restrict__ logits,
                                                                     const int64_t* __restrict__ target_a,
                                                                     const int64_t* __restrict__ target_b,
                                                                     const float* __restrict__ lam,
                                                                     float* __restrict__ ws, int B, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (int64_t)row * C;
  const int64_t a64 = target_a[row], b64 = target_b[row];
  const bool valid = a64 >= 0 && a64 < C && b64 >= 0 && b64 < C;
  const float xa = Cvt<T>::to_f32(x[valid ? (int)a64 : 0]);  // C >= 1: column 0 exists also for an ignored row
  const float xb = Cvt<T>::to_f32(x[valid ? (int)b64 : 0]);
  MixRowAcc a;
  if constexpr (kVec) {
    constexpr int N = Raw16<T>::kN;
    const int nvec = C / N;  // exact: the pitch is a multiple of 16 bytes
    for (int v0 = lane; v0 < nvec; v0 += 64 * kXUnroll) {
      Raw16<T> r[kXUnroll];
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u)
        if (v0 + 64 * u < nvec) r[u].load(x + (int64_t)(v0 + 64 * u) * N);
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u) {
        if (v0 + 64 * u >= nvec) break;
        float f[N];
        float vm = -INFINITY;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          f[j] = r[u].get(j);
          vm = fmaxf(vm, f[j]);
        }
        a.o.rescale(fmaxf(a.o.m, vm));
#pragma unroll
        for (int j = 0; j < N; ++j) {
          a.o.add(f[j]);
          a.sum += f[j];
        }
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float f = Cvt<T>::to_f32(x[c]);
      a.o.rescale(fmaxf(a.o.m, f));
      a.o.add(f);
      a.sum += f;
    }
  }
  const float m = wave_max(a.o.m);
  a.o.rescale(m);  // a lane still at -inf keeps its s (0, or NaN from a NaN logit)
  const float s = wave_sum(a.o.s);
  const float sum = wave_sum(a.sum);
  if (lane == 0) {
    const float lse = m + __logf(s);
    const float wa = lam[row], wb = 1.f - wa;
    // a weight of exactly 0 drops its term, so a -inf logit at that class does not turn 0 * inf into NaN
    const float xt = (wa != 0.f ? wa * xa : 0.f) + (wb != 0.f ? wb * xb : 0.f);
    const float smooth = eps > 0.f ? eps * (sum / (float)C) : 0.f;
    ws[row] = lse;
    ws[B + row] = valid ? lse - (1.f - eps) * xt - smooth : 0.f;
    ws[2 * B + row] = valid ? 1.f : 0.f;
  }
}

// stats = [sum of row losses over valid rows, valid rows]; ws[3 * B] = stats[0] / stats[1], the mean loss (NaN
// without a valid row). One workgroup, the order of xent_stats_kernel, no float atomics.
__global__ __launch_bounds__(256) void xent_mix_mean_kernel(float* __restrict__ ws, float* __restrict__ stats, int B) {
  __shared__ float red[2][4];
  float acc[2] = {0.f, 0.f};
  for (int i = threadIdx.x; i < B; i += 256) {
    acc[0] += ws[B + i];
    acc[1] += ws[2 * B + i];
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    acc[q] = wave_sum(acc[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      tot[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
      stats[q] = tot[q];
    }
    ws[3 * B] = tot[1] > 0.f ? tot[0] / tot[1] : NAN;
  }
}

template <typename T, bool kVec>
__global__ __launch_bounds__(kXWaves * 64) void xent_mix_bwd_kernel(const T* __restrict__ logits,
                                                                    const int64_t* __restrict__ target_a,
                                                                    const int64_t* __restrict__ target_b,
                                                                    const float* __restrict__ lam,
                                                                    const float* __restrict__ ws,
                                                                    const float* __restrict__ stats,
                                                                    const float* __restrict__ gout,
                                                                    T* __restrict__ dlogits, int B, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (int64_t)row * C;
  T* d = dlogits + (int64_t)row * C;
  const int64_t a64 = target_a[row], b64 = target_b[row];
  const bool valid = a64 >= 0 && a64 < C && b64 >= 0 && b64 < C;
  const int ta = valid ? (int)a64 : -1, tb = valid ? (int)b64 : -1;
  const float lse = ws[row];
  const float g = valid ? gout[0] / stats[1] : 0.f;  // one division per row
  const float wa = lam[row];
  const float hot = 1.f - eps, uni = eps / (float)C;
  const float ha = hot * wa, hb = hot * (1.f - wa);  // ta == tb: the two terms add
  if constexpr (kVec) {
    constexpr int N = Raw16<T>::kN;
    const int nvec = C / N;
    for (int v0 = lane; v0 < nvec; v0 += 64 * kXUnroll) {
      Raw16<T> r[kXUnroll];
      if (valid) {
#pragma unroll
        for (int u = 0; u < kXUnroll; ++u)
          if (v0 + 64 * u < nvec) r[u].load(x + (int64_t)(v0 + 64 * u) * N);
      }
#pragma unroll
      for (int u = 0; u < kXUnroll; ++u) {
        if (v0 + 64 * u >= nvec) break;
        const int c0 = (v0 + 64 * u) * N;
        Raw16<T> o;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const float h = (c0 + j == ta ? ha : 0.f) + (c0 + j == tb ? hb : 0.f);
          o.set(j, valid ? (__expf(r[u].get(j) - lse) - h - uni) * g : 0.f);
        }
        o.store(d + c0);
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      float v = 0.f;
      if (valid) {
        const float h = (c == ta ? ha : 0.f) + (c == tb ? hb : 0.f);
        v = (__expf(Cvt<T>::to_f32(x[c]) - lse) - h - uni) * g;
      }
      d[c] = Cvt<T>::from_f32(v);
    }
  }
}

static bool xent_rows_vectorisable(const void* p, int C, int dtype) {
  const size_t pitch = (size_t)C * (dtype == kF32 ? 4 : 2);
  return (reinterpret_cast<uintptr_t>(p) % 16 == 0) && (pitch % 16 == 0);
}

// One wave per row: launch(T tag, kVec constant, grid, block) for the logits' dtype and layout.
template <typename F>
static void xent_launch_rows(int B, int dtype, bool vec, F launch) {
  dim3 grid((B + kXWaves - 1) / kXWaves), block(kXWaves * 64);
  dispatch_dtype(dtype, vec, [&](auto t, auto v) { launch(t, v, grid, block); });
}

void launch_xent_metrics_fwd(const void* logits, const int64_t* target, float* ws, float* stats, int B, int C,
                             float eps, int k, int dtype, hipStream_t stream) {
  if (B > 0)
    xent_launch_rows(B, dtype, xent_rows_vectorisable(logits, C, dtype), [&](auto t, auto v, dim3 grid, dim3 block) {
      using T = tag_t<decltype(t)>;
      hipLaunchKernelGGL((xent_metric_rows_kernel<T, decltype(v)::value>), grid, block, 0, stream, (const T*)logits,
                         target, ws, B, C, eps);
    });
  hipLaunchKernelGGL(xent_stats_kernel, dim3(1), dim3(256), 0, stream, ws, stats, B, k);
}

void launch_xent_smooth_bwd(const void* logits, const int64_t* target, const float* ws, const float* stats,
                            const float* gout, void* dlogits, int B, int C, float eps, int dtype,
                            hipStream_t stream) {
  if (B <= 0) return;
  const bool vec = xent_rows_vectorisable(logits, C, dtype) && xent_rows_vectorisable(dlogits, C, dtype);
  xent_launch_rows(B, dtype, vec, [&](auto t, auto v, dim3 grid, dim3 block) {
    using T = tag_t<decltype(t)>;
    hipLaunchKernelGGL((xent_smooth_bwd_kernel<T, decltype(v)::value>), grid, block, 0, stream, (const T*)logits,
                       target, ws, stats, gout, (T*)dlogits, B, C, eps);
  });
}

void launch_xent_mix_fwd(const void* logits, const int64_t* target_a, const int64_t* target_b, const float* lam,
                         float* ws, float* stats, int B, int C, float eps, int dtype, hipStream_t stream) {
  if (B > 0)
    xent_launch_rows(B, dtype, xent_rows_vectorisable(logits, C, dtype), [&](auto t, auto v, dim3 grid, dim3 block) {
      using T = tag_t<decltype(t)>;
      hipLaunchKernelGGL((xent_mix_rows_kernel<T, decltype(v)::value>), grid, block, 0, stream, (const T*)logits,
                         target_a, target_b, lam, ws, B, C, eps);
    });
  hipLaunchKernelGGL(xent_mix_mean_kernel, dim3(1), dim3(256), 0, stream, ws, stats, B);
}

void launch_xent_mix_bwd(const void* logits, const int64_t* target_a, const int64_t* target_b, const float* lam,
                         const float* ws, const float* stats, const float* gout, void* dlogits, int B, int C,
                         float eps, int dtype, hipStream_t stream) {
  if (B <= 0) return;
  const bool vec = xent_rows_vectorisable(logits, C, dtype) && xent_rows_vectorisable(dlogits, C, dtype);
  xent_launch_rows(B, dtype, vec, [&](auto t, auto v, dim3 grid, dim3 block) {
    using T = tag_t<decltype(t)>;
    hipLaunchKernelGGL((xent_mix_bwd_kernel<T, decltype(v)::value>), grid, block, 0, stream, (const T*)logits,
                       target_a, target_b, lam, ws, stats, gout, (T*)dlogits, B, C, eps);
  });
}

}  // namespace dla
