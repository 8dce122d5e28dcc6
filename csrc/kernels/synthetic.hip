// On-device synthetic data.
//
// The reference draws `torch.rand_like(data)` / `torch.randint_like(target, high)` on the CPU
// every step and then copies the batch H2D (/root/reference/src/data.py:129-132,
// /root/reference/src/main.py:57,65): ~130 ms of a 403 ms P100 step.
// Here the batch is generated directly in HBM by a counter-based Philox-4x32-10 generator:
// every 64-bit output index maps to one counter, so any (seed, step) stream is reproducible
// and independent of the launch geometry. Write-bound: 128x3x224x224 bf16 = 38.5 MB ≈ 7 µs.
#include "dla_common.h"
#include "dla_kernels.h"

namespace dla {

struct Philox {
  static constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  __device__ __forceinline__ static void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)M0 * c[0];
    const uint64_t p1 = (uint64_t)M1 * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
  }
  __device__ __forceinline__ static void gen(uint64_t seed, uint64_t ctr, uint32_t (&out)[4]) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    out[0] = (uint32_t)ctr; out[1] = (uint32_t)(ctr >> 32); out[2] = 0x5eedu; out[3] = 0xda7au;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      round(out, k0, k1);
      k0 += W0; k1 += W1;
    }
  }
};

// [0, 1) with 24-bit resolution in fp32. A bf16 fill rounds this value to nearest, so it is in [0, 1]:
// a draw >= 1 - 2^-9 becomes exactly 1.0 (probability 2^-9 per element). The stream is kept as it is --
// recorded bf16 inputs depend on it -- and tests/test_gpu_synthetic.py pins both ranges.
__device__ __forceinline__ float u32_to_unit(uint32_t x) {
  return (x >> 8) * (1.0f / 16777216.0f);
}

// Stream position: offset + (*step) * per_step when `step` (a device counter) is given — a graph
// replay then draws a fresh batch each time without any host-side argument change.
__device__ __forceinline__ uint64_t stream_offset(uint64_t offset, const int64_t* step, uint64_t per_step) {
  return step ? offset + (uint64_t)(*step) * per_step : offset;
}

template <typename T>
__global__ __launch_bounds__(256) void uniform_kernel(T* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset,
                                                      float lo, float span, const int64_t* __restrict__ step,
                                                      uint64_t per_step) {
  offset = stream_offset(offset, step, per_step);
  const int64_t ngroups = (n + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += stride) {
    uint32_t r[4];
    Philox::gen(seed, offset + (uint64_t)gi, r);
    const int64_t i = gi * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = lo + span * u32_to_unit(r[j]);
    if (i + 4 <= n) {
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4_t*>(reinterpret_cast<float*>(out) + i) = float4_t{v[0], v[1], v[2], v[3]};
      } else {
        *reinterpret_cast<ushort4_t*>(reinterpret_cast<bf16_t*>(out) + i) =
            ushort4_t{f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])};
      }
    } else {
      for (int j = 0; j < 4 && i + j < n; ++j) out[i + j] = Cvt<T>::from_f32(v[j]);
    }
  }
}

__global__ __launch_bounds__(256) void randint_kernel(int64_t* __restrict__ out, int64_t n, int64_t high, uint64_t seed,
                                                      uint64_t offset, const int64_t* __restrict__ step,
                                                      uint64_t per_step) {
  offset = stream_offset(offset, step, per_step);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint32_t r[4];
    Philox::gen(seed ^ 0x1abe1ull, offset + (uint64_t)i, r);
    const uint64_t x = ((uint64_t)r[0] << 32) | r[1];
    out[i] = (int64_t)(x % (uint64_t)high);
  }
}

void launch_uniform_fill(void* out, int64_t n, int dtype, uint64_t seed, uint64_t offset, float lo, float hi,
                         hipStream_t stream, const int64_t* step, uint64_t per_step) {
  if (n <= 0) return;
  int64_t groups = (n + 3) / 4;
  int grid = (int)std::min<int64_t>((groups + 255) / 256, 4096);
  if (dtype == kF32)
    hipLaunchKernelGGL(uniform_kernel<float>, dim3(grid), dim3(256), 0, stream, (float*)out, n, seed, offset, lo, hi - lo,
                       step, per_step);
  else
    hipLaunchKernelGGL(uniform_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (bf16_t*)out, n, seed, offset, lo,
                       hi - lo, step, per_step);
}

void launch_randint_fill(int64_t* out, int64_t n, int64_t high, uint64_t seed, uint64_t offset, hipStream_t stream,
                         const int64_t* step, uint64_t per_step) {
  if (n <= 0) return;
  int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(randint_kernel, dim3(grid), dim3(256), 0, stream, out, n, high, seed, offset, step, per_step);
}

}  // namespace dla
