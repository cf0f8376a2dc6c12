// Fused image-batch preparation: crop -> antialiased bilinear resize ->
// window -> mirror -> normalise -> cast -> NHWC, one launch per batch.
//
// Images live packed back to back in one uint8 arena (HWC RGB, no alignment
// promised for an image's start). Per sample the host supplies the source
// box, the size the box is virtually resized to, and the out_size x out_size
// window taken from that virtual image, so "crop then resize" (train) and
// "resize then centre crop" (val) are the same geometry.
//
// Sampling rule per axis (PIL / ATen antialiased bilinear), `in` the box
// extent and `out` the virtual extent:
//   scale = in / out, fs = max(scale, 1), center = scale * (o + 0.5)
//   lo = max(0, int(center - fs + 0.5)), hi = min(in, int(center + fs + 0.5))
//   w_j = max(0, 1 - |(j - center + 0.5) / fs|), normalised to sum 1
// The tap count grows with the downscale factor, so both axes are loops.
//
// Mapping: grid.y = sample (metadata is block-uniform and lands in SGPRs),
// each thread owns kPix consecutive output pixels x 3 channels, which are
// contiguous in NHWC: 24 B (16-bit) or 48 B (fp32) per thread, written with
// 8 B / 16 B vector stores whenever S*S is a multiple of kPix.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPix = 4;    // output pixels per thread
constexpr int kMeta = 11;  // H W x0 y0 bw bh oh ow oy ox flip

struct Norm {
  float sub[3];  // 255 * mean
  float mul[3];  // 1 / (255 * std)
};

struct Axis {
  int lo, hi;
  float center, inv_fs, inv_sum;
};

DEV_INLINE float tap_w(const Axis& a, int j) {
  return fmaxf(0.0f, 1.0f - fabsf(((float)j - a.center + 0.5f) * a.inv_fs));
}

DEV_INLINE Axis axis_taps(int in, int out, int o) {
  Axis a;
  float scale = (float)in / (float)out;
  float fs = fmaxf(scale, 1.0f);
  a.center = scale * ((float)o + 0.5f);
  a.inv_fs = 1.0f / fs;
  a.lo = max(0, (int)(a.center - fs + 0.5f));
  a.hi = min(in, (int)(a.center + fs + 0.5f));
  // taps never leave the box, whatever the window asked for
  a.lo = min(a.lo, in - 1);
  a.hi = max(a.hi, a.lo + 1);
  float sum = 0.0f;
  for (int j = a.lo; j < a.hi; ++j) sum += tap_w(a, j);
  a.inv_sum = sum > 0.0f ? 1.0f / sum : 0.0f;
  return a;
}

// Block-uniform view of one sample: the clamped box and the geometry.
struct Sample {
  const uint8_t* img;  // first byte of the box
  int64_t row_stride;  // bytes per image row
  int bw, bh, oh, ow, oy, ox, flip;
  bool ok;
};

// One output pixel (flat index p in the S x S window), 3 channels.
template <typename T>
DEV_INLINE void pixel(const Sample& s, const Norm& nm, int S, int npix, int p,
                      T* v) {
  float r = 0.0f, g = 0.0f, bl = 0.0f, k = 0.0f;
  if (s.ok && p < npix) {
    const int yo = p / S;
    const int xo = p - yo * S;
    const int xw = s.flip ? S - 1 - xo : xo;
    const Axis ay = axis_taps(s.bh, s.oh, s.oy + yo);
    const Axis ax = axis_taps(s.bw, s.ow, s.ox + xw);
    for (int y = ay.lo; y < ay.hi; ++y) {
      const float wy = tap_w(ay, y);
      const uint8_t* px = s.img + (int64_t)y * s.row_stride + ax.lo * 3;
      float rr = 0.0f, gg = 0.0f, bb = 0.0f;
      for (int x = ax.lo; x < ax.hi; ++x, px += 3) {
        const float wx = tap_w(ax, x);
        rr += wx * (float)px[0];
        gg += wx * (float)px[1];
        bb += wx * (float)px[2];
      }
      r += wy * rr;
      g += wy * gg;
      bl += wy * bb;
    }
    k = ay.inv_sum * ax.inv_sum;
  }
  v[0] = from_f32<T>((r * k - nm.sub[0]) * nm.mul[0]);
  v[1] = from_f32<T>((g * k - nm.sub[1]) * nm.mul[1]);
  v[2] = from_f32<T>((bl * k - nm.sub[2]) * nm.mul[2]);
}

template <typename T, typename V>
__global__ __launch_bounds__(kBlock) void crop_resize_kernel(
    const uint8_t* __restrict__ arena, int64_t arena_bytes,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ meta,
    T* __restrict__ out, int S, Norm nm, int vec) {
  const int b = blockIdx.y;
  const int npix = S * S;
  const int p0 = (blockIdx.x * kBlock + threadIdx.x) * kPix;
  if (p0 >= npix) return;

  const int32_t* m = meta + (int64_t)b * kMeta;
  int H = m[0], W = m[1], x0 = m[2], y0 = m[3];
  const int64_t off = offsets[b];

  // The host validates every request; this is the second fence. A sample
  // whose image does not lie in the arena produces zeros, and the box is
  // clamped into the image so no tap can address outside it.
  Sample s;
  s.oh = m[6]; s.ow = m[7]; s.oy = m[8]; s.ox = m[9]; s.flip = m[10];
  s.ok = H >= 1 && W >= 1 && s.oh >= 1 && s.ow >= 1 && off >= 0 &&
         off + 3 * (int64_t)H * W <= arena_bytes;
  if (!s.ok) { H = 1; W = 1; s.oh = 1; s.ow = 1; }
  x0 = min(max(x0, 0), W - 1);
  y0 = min(max(y0, 0), H - 1);
  s.bw = min(max(m[4], 1), W - x0);
  s.bh = min(max(m[5], 1), H - y0);
  s.img = arena + (s.ok ? off : 0) + ((int64_t)y0 * W + x0) * 3;
  s.row_stride = (int64_t)W * 3;

  // four explicit calls, not a loop over an array: the values stay in VGPRs
  static_assert(kPix == 4, "one pixel() call per owned pixel");
  union {
    T vals[kPix * 3];
    V pack[3];
  } u;
  pixel<T>(s, nm, S, npix, p0 + 0, u.vals + 0);
  pixel<T>(s, nm, S, npix, p0 + 1, u.vals + 3);
  pixel<T>(s, nm, S, npix, p0 + 2, u.vals + 6);
  pixel<T>(s, nm, S, npix, p0 + 3, u.vals + 9);

  T* dst = out + ((int64_t)b * npix + p0) * 3;
  if (vec) {
    // S*S % kPix == 0: the group is whole and its start is sizeof(V)-aligned
    static_assert(sizeof(u.vals) == sizeof(u.pack), "store width");
    V* d = reinterpret_cast<V*>(dst);
    d[0] = u.pack[0];
    d[1] = u.pack[1];
    d[2] = u.pack[2];
  } else {
    const int n = min(kPix, npix - p0) * 3;
#pragma unroll
    for (int i = 0; i < kPix * 3; ++i)
      if (i < n) dst[i] = u.vals[i];
  }
}

template <typename T, typename V>
void launch(const torch::Tensor& arena, const torch::Tensor& offsets,
            const torch::Tensor& meta, torch::Tensor& out, int B, int S,
            const Norm& nm) {
  const int npix = S * S;
  const int vec = (npix % kPix) == 0;
  dim3 grid((npix + kBlock * kPix - 1) / (kBlock * kPix), B);
  hipLaunchKernelGGL((crop_resize_kernel<T, V>), grid, dim3(kBlock), 0,
                     c10::hip::getCurrentHIPStream(),
                     arena.data_ptr<uint8_t>(), (int64_t)arena.numel(),
                     offsets.data_ptr<int64_t>(), meta.data_ptr<int32_t>(),
                     (T*)out.data_ptr(), S, nm, vec);
}

}  // namespace

// out_dtype: 0 = fp32, 1 = bf16, 2 = fp16
torch::Tensor crop_resize_mirror_normalize(torch::Tensor arena,
                                           torch::Tensor offsets,
                                           torch::Tensor meta,
                                           int64_t out_size,
                                           std::vector<double> mean,
                                           std::vector<double> std,
                                           int64_t out_dtype) {
  TORCH_CHECK(arena.is_cuda() && offsets.is_cuda() && meta.is_cuda(),
              "crop_resize_mirror_normalize: tensors must be on the GPU");
  TORCH_CHECK(arena.get_device() == offsets.get_device() &&
              arena.get_device() == meta.get_device(),
              "crop_resize_mirror_normalize: tensors on different devices");
  TORCH_CHECK(arena.scalar_type() == at::kByte && arena.dim() == 1 &&
              arena.is_contiguous(), "arena must be contiguous 1-D uint8");
  TORCH_CHECK(offsets.scalar_type() == at::kLong && offsets.dim() == 1 &&
              offsets.is_contiguous(), "offsets must be contiguous int64[B]");
  const int64_t B = offsets.size(0);
  TORCH_CHECK(meta.scalar_type() == at::kInt && meta.dim() == 2 &&
              meta.size(0) == B && meta.size(1) == kMeta &&
              meta.is_contiguous(), "meta must be contiguous int32[B, 11]");
  TORCH_CHECK(out_size >= 1 && out_size <= 16384, "out_size out of range");
  TORCH_CHECK(B <= 65535, "batch too large for one launch");
  TORCH_CHECK(mean.size() == 3 && std.size() == 3, "mean/std need 3 values");
  TORCH_CHECK(out_dtype >= 0 && out_dtype <= 2, "out_dtype must be 0, 1 or 2");

  Norm nm;
  for (int c = 0; c < 3; ++c) {
    TORCH_CHECK(std[c] > 0.0, "std must be positive");
    nm.sub[c] = (float)(255.0 * mean[c]);
    nm.mul[c] = (float)(1.0 / (255.0 * std[c]));
  }
  const at::ScalarType dt = out_dtype == 0 ? at::kFloat
                            : out_dtype == 1 ? at::kBFloat16 : at::kHalf;
  const int S = (int)out_size;
  auto out = torch::empty({B, 3, S, S},
                          arena.options().dtype(dt).memory_format(
                              at::MemoryFormat::ChannelsLast));
  if (B == 0) return out;
  if (out_dtype == 0)
    launch<float, float4>(arena, offsets, meta, out, (int)B, S, nm);
  else if (out_dtype == 1)
    launch<__hip_bfloat16, uint2>(arena, offsets, meta, out, (int)B, S, nm);
  else
    launch<_Float16, uint2>(arena, offsets, meta, out, (int)B, S, nm);
  HIP_CHECK_LAST();
  return out;
}
