// Training augmentation from raw uint8 batches, one pass: per-sample crop, bilinear resample, horizontal
// flip, normalise, cast and channels-last layout.
//
// src [N][Hs][Ws][3] uint8 -> out dense [N][Ho][Wo][3] (the memory of a channels_last [N,3,Ho,Wo] tensor,
// what SyntheticBatches writes), bf16 or fp32. Per sample n: geom[n] = (y0, x0, step_y, step_x) in source
// pixels and flip[n]. Output pixel (n, oy, ox, c), all in fp32:
//   ox' = flip ? Wo-1-ox : ox;  sy = (y0 - 0.5) + (oy + 0.5) * step_y;  sx likewise with ox'
//   taps floor(s), floor(s)+1, each clamped to [-pad, size-1+pad]; a tap outside [0, size) reads 0
//   v = bilinear blend with weights (1-fy, fy) x (1-fx, fx);  out = fmaf(v, scale[c], bias[c])
// pad = 0 clamps at the edges (random-resized crop); pad = p with step 1 and integer offsets in [-p, p] is a
// crop of the image padded with p black pixels. At step 1 and integer offsets fy = fx = 0, the blend is
// one source byte and the result is fmaf(byte, scale, bias) exactly.
//
// The output is walked linearly in 16-byte groups anchored at the 16-byte boundary at or before `out`: a
// group that lies inside the tensor is one 16-byte store per lane (8 bf16 / 4 fp32), the (at most two) groups
// that hang over either end store their valid elements one by one -- so neither the base address, an image's
// element count nor a row has to be a multiple of the vector width.
//
// A group of V elements starts at channel c0 of some pixel and touches at most kPix = (V + 4) / 3 pixels.
// Every lane computes all three channels of those kPix pixels -- the same straight-line code whatever c0 is,
// no divergence inside a wave -- and then picks its V values at offset c0. The kernel is bound by the
// instructions it issues, not by bytes (profiles/augment/README.md), so memory instructions are kept few: a
// pixel costs two source loads -- the six bytes of a row's two x taps, which are neighbours, come from one
// unaligned 8-byte load -- and geom and flip are loaded once per group and again only where it runs into
// the next image.
//
// Mixed forms (Mixup / CutMix, launch_augment_mix): per sample a partner image p, a weight lam and a box
// (y0, x0, y1, x1) on the output grid. With A(j) the value above for source image j with ITS geom and flip,
//   w = inside the box ? 0 : lam[n];   out = fmaf(w, A(n), (1 - w) * A(p))
// kSelect needs lam == 1 everywhere: w is 0 or 1, so a pixel is sampled once, from image n or p -- the plain
// kernel's count of source loads. kBlend samples both and is valid for any parameters. partner, lam, box and
// the partner's geom and flip are loaded once per group and again where it runs into the next image, like
// geom. The plain instantiation has none of this.
//
// Indexed forms (launch_augment_gather, launch_augment_mix_gather): src is a resident store [P][Hs][Ws][3] that
// may hold far more than 2^31 bytes, and batch image n is store row r(n) = min(uint32(index[n]), P - 1); the
// partner of n is row r(partner[n]), with the geom and flip of batch position partner[n]. An image is addressed
// by a 64-bit base, src + r * (Hs * Ws * 3), formed where geom is loaded (once per group, again where it runs
// into the next image); offsets inside the image stay 32-bit and the 8-byte load is clamped at the image's own
// last 8 bytes. The six bytes of a row's two x taps never leave an image, so the bytes extracted are the ones
// the plain kernel extracts from store[index]. The instantiations without kGather have none of this.
#include "dla_common.h"
#include "dla_kernels.h"

namespace dla {

struct AugmentArgs {
  const uint8_t* src;
  const float* geom;    // [N][4], 16-byte aligned
  const uint8_t* flip;  // [N]
  const float* scale;   // [3]
  const float* bias;    // [3]
  uint32_t total;       // N * Ho * Wo * 3, < 2^31
  uint32_t shift;       // elements between the 16-byte boundary at or before `out` and `out`
  uint32_t last8;       // N * Hs * Ws * 3 - 8: the last byte offset an 8-byte load may start at (indexed forms:
                        // Hs * Ws * 3 - 8, relative to the image)
  int Hs, Ws, Ho, Wo, pad;
  // mixed forms only (null in the plain launch)
  const int32_t* partner;  // [N], in [0, N)
  const float* lam;        // [N], in [0, 1]
  const int32_t* box;      // [N][4] = (y0, x0, y1, x1) on the output grid, 16-byte aligned
  uint32_t nimg;           // N
  // indexed forms only (null in the others)
  const int32_t* index;  // [N], in [0, P)
  uint32_t nrows;        // P
  uint32_t imgbytes;     // Hs * Ws * 3, < 2^31
};

enum AugmentMode { kPlain = 0, kSelect = 1, kBlend = 2 };
typedef int int4_t __attribute__((ext_vector_type(4)));

constexpr float kFar = 1073741824.f;  // 2^30

// tap t of an axis of `size` source pixels: clamped to the padded range; `inside` false = reads black
__device__ __forceinline__ int clamp_tap(int t, int size, int pad, bool& inside) {
  t = max(-pad, min(t, size - 1 + pad));
  inside = t >= 0 && t < size;
  return inside ? t : 0;
}

// Both x taps of one source row: the pixel at byte offset `off` (low 24 bits of .x) and, when `next`, the
// pixel after it (.y; else the same pixel again). One unaligned 8-byte load; it starts at min(off, last8) so
// that it never reaches past the tensor's last byte: the six bytes of two pixels end at most at the
// tensor's end, so off - last8 <= 2 then, and <= 5 when only the tensor's last pixel is wanted.
struct TapPair {
  uint32_t x, y;
};
__device__ __forceinline__ TapPair load_pair(const uint8_t* __restrict__ src, uint32_t off, uint32_t last8, bool next) {
  const uint32_t at = min(off, last8);
  uint64_t u;
  __builtin_memcpy(&u, src + at, 8);
  u >>= 8u * (off - at);
  const uint32_t a = (uint32_t)u;
  return TapPair{a, next ? (uint32_t)(u >> 24) : a};
}

__device__ __forceinline__ float channel(uint32_t rgb, int c) { return (float)((rgb >> (8 * c)) & 0xffu); }

// The first byte of the store row that batch position n reads (indexed forms); a bad index cannot leave the store.
__device__ __forceinline__ const uint8_t* store_row(const AugmentArgs& a, uint32_t n) {
  return a.src + (size_t)min((uint32_t)a.index[n], a.nrows - 1u) * a.imgbytes;
}

// All three channels of output pixel (oy, ox) sampled from source image `img` of `src` with that image's geom and
// flip. The indexed forms pass the image's own first byte as `src` and img = 0.
__device__ __forceinline__ void sample_pixel(const AugmentArgs& a, const uint8_t* __restrict__ src, uint32_t img,
                                             int oy, int ox, const float4_t gm,
                                             uint32_t fl, const float (&sc)[3], const float (&bi)[3], float* val) {
  const int oxs = fl ? a.Wo - 1 - ox : ox;
  const float sy = (gm.x - 0.5f) + ((float)oy + 0.5f) * gm.z;
  const float sx = (gm.y - 0.5f) + ((float)oxs + 0.5f) * gm.w;
  // taps far outside clamp to the border anyway; bounding them first keeps the int conversion defined
  const float ty = fminf(fmaxf(floorf(sy), -kFar), kFar), tx = fminf(fmaxf(floorf(sx), -kFar), kFar);
  const float fy = sy - ty, fx = sx - tx;
  bool iy0, iy1, ix0, ix1;
  const int y0 = clamp_tap((int)ty, a.Hs, a.pad, iy0), y1 = clamp_tap((int)ty + 1, a.Hs, a.pad, iy1);
  const int x0 = clamp_tap((int)tx, a.Ws, a.pad, ix0), x1 = clamp_tap((int)tx + 1, a.Ws, a.pad, ix1);
  // byte offsets stay below N * Hs * Ws * 3 < 2^31 (indexed forms: below Hs * Ws * 3)
  const uint32_t r0 = (img * (uint32_t)a.Hs + (uint32_t)y0) * (uint32_t)a.Ws;
  const uint32_t r1 = (img * (uint32_t)a.Hs + (uint32_t)y1) * (uint32_t)a.Ws;
  // two x taps that are both inside are the same pixel (clamped at an edge) or neighbours; a tap outside
  // has weight 0 below, so what is read for it does not matter
  const bool next = x1 != x0;
  const TapPair q0 = load_pair(src, (r0 + (uint32_t)x0) * 3u, a.last8, next);
  const TapPair q1 = load_pair(src, (r1 + (uint32_t)x0) * 3u, a.last8, next);
  const uint32_t q00 = q0.x, q01 = q0.y, q10 = q1.x, q11 = q1.y;
  const float w00 = iy0 && ix0 ? (1.f - fy) * (1.f - fx) : 0.f, w01 = iy0 && ix1 ? (1.f - fy) * fx : 0.f;
  const float w10 = iy1 && ix0 ? fy * (1.f - fx) : 0.f, w11 = iy1 && ix1 ? fy * fx : 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float blend =
        (w00 * channel(q00, c) + w01 * channel(q01, c)) + (w10 * channel(q10, c) + w11 * channel(q11, c));
    val[c] = fmaf(blend, sc[c], bi[c]);
  }
}

// What a mixed group knows about image n's partner.
struct MixState {
  uint32_t p;    // partner image, clamped into the batch so that a bad index cannot read outside geom / flip
  float lam;
  int4_t box;
  float4_t gm;   // the partner's geom
  uint32_t fl;   // and flip
  const uint8_t* base;  // indexed forms: the partner's store row
  template <bool kGather>
  __device__ __forceinline__ void load(const AugmentArgs& a, uint32_t n) {
    p = min((uint32_t)a.partner[n], a.nimg - 1u);
    lam = a.lam[n];
    box = *reinterpret_cast<const int4_t*>(a.box + 4 * (size_t)n);
    gm = *reinterpret_cast<const float4_t*>(a.geom + 4 * (size_t)p);
    fl = a.flip[p];
    if constexpr (kGather) base = store_row(a, p);
  }
  __device__ __forceinline__ bool inbox(int oy, int ox) const {
    return oy >= box.x && oy < box.z && ox >= box.y && ox < box.w;
  }
};

template <typename T, int kMode, bool kGather = false>
__global__ __launch_bounds__(256) void augment_kernel(T* __restrict__ out, const AugmentArgs a) {
  constexpr int V = 16 / sizeof(T);
  constexpr int kPix = (V + 4) / 3;  // pixels a group can touch: V elements from channel 2 on
  const uint32_t ngroups = (a.total + a.shift + V - 1) / V;
  const uint32_t npix = a.total / 3u;
  const uint32_t stride = gridDim.x * blockDim.x;
  const float sc[3] = {a.scale[0], a.scale[1], a.scale[2]};
  const float bi[3] = {a.bias[0], a.bias[1], a.bias[2]};
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += stride) {
    // elements [lo, hi) of the tensor; v[j] is element lo + j
    const int64_t first = (int64_t)g * V - a.shift;
    const uint32_t lo = first < 0 ? 0u : (uint32_t)first;
    const uint32_t hi = min((uint32_t)(first + V), a.total);
    const uint32_t p0 = lo / 3u;
    const uint32_t c0 = lo - p0 * 3u;
    const uint32_t row = p0 / (uint32_t)a.Wo;
    int ox = (int)(p0 - row * (uint32_t)a.Wo);
    uint32_t n = row / (uint32_t)a.Ho;
    int oy = (int)(row - n * (uint32_t)a.Ho);

    float val[kPix * 3];  // channels of pixels p0 .. p0 + kPix - 1
    uint32_t gn = n;      // the image gm and fl belong to: reloaded where a group runs into the next image
    float4_t gm = *reinterpret_cast<const float4_t*>(a.geom + 4 * (size_t)n);
    uint32_t fl = a.flip[n];
    MixState mx;
    if constexpr (kMode != kPlain) mx.template load<kGather>(a, n);
    // the image n is read from: the batch itself, or (indexed forms) n's store row as image 0 of its own base
    const uint8_t* sb = a.src;
    if constexpr (kGather) sb = store_row(a, n);
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      if (n != gn) {
        gn = n;
        gm = *reinterpret_cast<const float4_t*>(a.geom + 4 * (size_t)n);
        fl = a.flip[n];
        if constexpr (kMode != kPlain) mx.template load<kGather>(a, n);
        if constexpr (kGather) sb = store_row(a, n);
      }
      const uint32_t own_img = kGather ? 0u : n;
      if constexpr (kMode == kPlain) {
        sample_pixel(a, sb, own_img, oy, ox, gm, fl, sc, bi, val + 3 * k);
      } else if constexpr (kMode == kSelect) {
        // lam == 1: the weight is 0 inside the box and 1 outside, so one of the two images is the result
        const bool in = mx.inbox(oy, ox);
        const float4_t sg = {in ? mx.gm.x : gm.x, in ? mx.gm.y : gm.y, in ? mx.gm.z : gm.z, in ? mx.gm.w : gm.w};
        if constexpr (kGather)
          sample_pixel(a, in ? mx.base : sb, 0u, oy, ox, sg, in ? mx.fl : fl, sc, bi, val + 3 * k);
        else
          sample_pixel(a, sb, in ? mx.p : n, oy, ox, sg, in ? mx.fl : fl, sc, bi, val + 3 * k);
      } else {
        float own[3], oth[3];
        sample_pixel(a, sb, own_img, oy, ox, gm, fl, sc, bi, own);
        if constexpr (kGather)
          sample_pixel(a, mx.base, 0u, oy, ox, mx.gm, mx.fl, sc, bi, oth);
        else
          sample_pixel(a, sb, mx.p, oy, ox, mx.gm, mx.fl, sc, bi, oth);
        const float w = mx.inbox(oy, ox) ? 0.f : mx.lam;
#pragma unroll
        for (int c = 0; c < 3; ++c) val[3 * k + c] = fmaf(w, own[c], (1.f - w) * oth[c]);
      }
      // the next pixel, unless this was the tensor's last one (then it is computed again and never used)
      if (p0 + k + 1 < npix && ++ox == a.Wo) {
        ox = 0;
        if (++oy == a.Ho) { oy = 0; ++n; }
      }
    }
    float v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = c0 == 0 ? val[j] : (c0 == 1 ? val[j + 1] : val[j + 2]);

    if (first >= 0 && first + V <= (int64_t)a.total) {
      T* dst = out + first;  // 16-byte aligned by the choice of shift
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4_t*>(dst) = float4_t{v[0], v[1], v[2], v[3]};
      } else {
        ushort8_t x;
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = f32_to_bf16(v[j]);
        *reinterpret_cast<ushort8_t*>(dst) = x;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (lo + j < hi) out[lo + j] = Cvt<T>::from_f32(v[j]);
    }
  }
}

// kGather: `a.index` and `a.nrows` are set by the caller and src is the store.
template <int kMode, bool kGather = false>
static void launch_augment_mode(const uint8_t* src, void* out, int dtype, AugmentArgs a, int N, int Hs, int Ws, int Ho,
                                int Wo, int pad, hipStream_t stream) {
  const int64_t total = (int64_t)N * Ho * Wo * 3;
  if (total <= 0) return;
  a.src = src;
  a.total = (uint32_t)total;
  const int esize = dtype == kF32 ? 4 : 2;
  a.shift = (uint32_t)(((uintptr_t)out & 15) / esize);
  // the caller guarantees at least three source pixels
  a.imgbytes = kGather ? (uint32_t)((int64_t)Hs * Ws * 3) : 0u;
  a.last8 = kGather ? a.imgbytes - 8u : (uint32_t)((int64_t)N * Hs * Ws * 3 - 8);
  a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo; a.pad = pad;
  a.nimg = (uint32_t)N;
  const int V = 16 / esize;
  const int64_t groups = (total + a.shift + V - 1) / V;
  const int grid = (int)std::min<int64_t>((groups + 255) / 256, 256 * 32);
  if (dtype == kF32)
    hipLaunchKernelGGL((augment_kernel<float, kMode, kGather>), dim3(grid), dim3(256), 0, stream, (float*)out, a);
  else
    hipLaunchKernelGGL((augment_kernel<bf16_t, kMode, kGather>), dim3(grid), dim3(256), 0, stream, (bf16_t*)out, a);
}

void launch_augment(const uint8_t* src, void* out, int dtype, const float* geom, const uint8_t* flip,
                    const float* scale, const float* bias, int N, int Hs, int Ws, int Ho, int Wo, int pad,
                    hipStream_t stream) {
  AugmentArgs a{};
  a.geom = geom;
  a.flip = flip;
  a.scale = scale;
  a.bias = bias;
  launch_augment_mode<kPlain>(src, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
}

void launch_augment_mix(const uint8_t* src, void* out, int dtype, const float* geom, const uint8_t* flip,
                        const int32_t* partner, const float* lam, const int32_t* box, const float* scale,
                        const float* bias, int N, int Hs, int Ws, int Ho, int Wo, int pad, bool blend,
                        hipStream_t stream) {
  AugmentArgs a{};
  a.geom = geom;
  a.flip = flip;
  a.scale = scale;
  a.bias = bias;
  a.partner = partner;
  a.lam = lam;
  a.box = box;
  if (blend)
    launch_augment_mode<kBlend>(src, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
  else
    launch_augment_mode<kSelect>(src, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
}

void launch_augment_gather(const uint8_t* store, int64_t P, const int32_t* index, void* out, int dtype,
                           const float* geom, const uint8_t* flip, const float* scale, const float* bias, int N,
                           int Hs, int Ws, int Ho, int Wo, int pad, hipStream_t stream) {
  AugmentArgs a{};
  a.geom = geom;
  a.flip = flip;
  a.scale = scale;
  a.bias = bias;
  a.index = index;
  a.nrows = (uint32_t)P;
  launch_augment_mode<kPlain, true>(store, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
}

void launch_augment_mix_gather(const uint8_t* store, int64_t P, const int32_t* index, void* out, int dtype,
                               const float* geom, const uint8_t* flip, const int32_t* partner, const float* lam,
                               const int32_t* box, const float* scale, const float* bias, int N, int Hs, int Ws,
                               int Ho, int Wo, int pad, bool blend, hipStream_t stream) {
  AugmentArgs a{};
  a.geom = geom;
  a.flip = flip;
  a.scale = scale;
  a.bias = bias;
  a.partner = partner;
  a.lam = lam;
  a.box = box;
  a.index = index;
  a.nrows = (uint32_t)P;
  if (blend)
    launch_augment_mode<kBlend, true>(store, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
  else
    launch_augment_mode<kSelect, true>(store, out, dtype, a, N, Hs, Ws, Ho, Wo, pad, stream);
}

}  // namespace dla
