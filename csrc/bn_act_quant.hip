// BN + ReLU + clip + fake-quantise (+ channel padding, + max) in one forward
// pass: the glue between a pooled conv output and the next noisy conv.
//
// The composition bn_act_fwd -> fake_quant_fwd -> max() -> pad_cols8 walks one
// large NHWC tensor seven times (read x, write A; read A, write Q; read Q;
// read Q, write Q padded). bn_act_quant_fwd reads x once and writes the
// activation A (the backward kernels, ste_mask and bn_act_bwd, read it), the
// [rows, C_pad] channel-padded quantised tensor the patch conv stages from,
// and the maximum of the quantised values. The unpadded quantised tensor is
// never stored.
//
// Every value is bit-identical to the composition: the stored activation
// comes from bn_act_value (common.h), and the stochastic-rounding draw of the
// element at flat index i of the UNPADDED tensor is lane i & 3 of
// philox4x32(seed, i >> 2) as in fake_quant_vec_kernel. Bit-identity also
// fixes every rounding, and the composition's kernels leave FMA contraction to
// the compiler, so the arithmetic here is written with contraction off and
// explicit FMAs, in the form fake_quant_vec_kernel's gfx950 code has: the
// scaled value and the rounding offset are rounded apart, then added. (The scalar
// quantiser that the composition runs at numel % 4 != 0 fuses the offset
// product for some lanes; the Python wrapper sends those sizes to the
// composition.) 16-bit dtypes only.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kFwdGridCap = 2048;   // slab-stride loop beyond this

template <typename T>
struct alignas(16) Pack8 { T v[8]; };

template <typename scalar_t> struct DevT { using type = scalar_t; };
template <> struct DevT<at::BFloat16> { using type = __hip_bfloat16; };
template <> struct DevT<at::Half> { using type = _Float16; };

// Per-channel constants live in LDS as separate arrays. Lane l of a wave
// works on channels 8*l.. (one 16-byte chunk each), so the plain index would
// put eight lanes on every bank; one skipped word per 8 channels spreads the
// stride-8 pattern over all banks.
DEV_INLINE int pidx(int c) { return c + (c >> 3); }
inline int pstride(int C) { return C + (C >> 3) + 1; }

// fake_quant of one stored activation, statement for statement as in
// fake_quant_vec_kernel
template <typename T, bool STOCH>
DEV_INLINE T quant_value(T a, float u, float min_value, float inv_scale,
                         float scale, float qmax) {
  // fake_quant_vec_kernel: the product and the offset are rounded apart.
  // (__fmul_rn / __fadd_rn are plain * and + in HIP and would be contracted
  // into one FMA; the pragma is what keeps the two roundings.)
#pragma clang fp contract(off)
  float q = (to_f32(a) - min_value) * inv_scale;
  if (STOCH) q = q + u;
  q = fminf(fmaxf(q, 0.0f), qmax);
  q = nearbyintf(q);
  return from_f32<T>(__fmaf_rn(q, scale, min_value));
}

// one stochastic-rounding offset, as fake_quant_vec_kernel forms it
DEV_INLINE float quant_offset(uint32_t r, float stoch) {
#pragma clang fp contract(off)
  return __fmaf_rn(2.0f, u01(r), -1.0f) * stoch;
}

// Forward. Each block takes slabs of slab_rows rows (a multiple of 8, so a
// slab starts on a 16-byte boundary and on a Philox quad of the flat
// tensor), walks the slab's flat element range in 8-element chunks with a
// running channel counter, and either stores the quantised values in place
// (C_pad == C) or parks them in LDS and writes the slab out row by row with
// channels C..C_pad-1 zero; the activation goes out in place either way.
// Dynamic LDS: 4 * ps floats of constants, then slab_rows * C elements when
// padding.
template <typename T, bool STOCH, bool PAD>
__global__ void bn_act_quant_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ act, T* __restrict__ out,
    int* __restrict__ max_bits,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    int64_t rows, int C, int C_pad, int slab_rows, int ps, int do_relu,
    float act_max, float min_value, float inv_scale, float scale, float qmax,
    float stoch, uint64_t seed, const int64_t* __restrict__ seed_base) {
  extern __shared__ __align__(16) char smem[];
  __shared__ float wmax[kBlock / WAVE];
  float* p_mean = (float*)smem;
  float* p_is = p_mean + ps;
  float* p_ga = p_is + ps;
  float* p_be = p_ga + ps;
  T* slab = (T*)(smem + (((size_t)4 * ps * sizeof(float) + 15) & ~(size_t)15));
  for (int c = threadIdx.x; c < C; c += kBlock) {
    p_mean[pidx(c)] = mean[c];
    p_is[pidx(c)] = invstd[c];
    p_ga[pidx(c)] = gamma[c];
    p_be[pidx(c)] = beta[c];
  }
  __syncthreads();
  seed = graph_seed(seed_base, seed);
  const int nchunks = C_pad >> 3;
  const int cstep = (kBlock * 8) % C;
  float vmax = 0.0f;  // the quantised values are >= 0 (relu, min_value == 0)
  for (int64_t r0 = (int64_t)blockIdx.x * slab_rows; r0 < rows;
       r0 += (int64_t)gridDim.x * slab_rows) {
    const int64_t e0 = r0 * C;
    const int64_t r1 = r0 + slab_rows < rows ? r0 + slab_rows : rows;
    const int64_t e1 = r1 * C;
    int c = (threadIdx.x * 8) % C;
    for (int64_t e = e0 + (int64_t)threadIdx.x * 8; e < e1;
         e += kBlock * 8) {
      const bool full = e + 8 <= e1;
      Pack8<T> xv;
      if (full) {
        xv = *(const Pack8<T>*)(x + e);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xv.v[j] = (e + j < e1) ? x[e + j] : from_f32<T>(0.0f);
      }
      float u[8] = {};
      if (STOCH) {
        Philox4 ph = philox4x32(seed, (uint64_t)(e >> 2));
        u[0] = quant_offset(ph.x, stoch);
        u[1] = quant_offset(ph.y, stoch);
        u[2] = quant_offset(ph.z, stoch);
        u[3] = quant_offset(ph.w, stoch);
        if (e + 4 < e1) {
          ph = philox4x32(seed, (uint64_t)(e >> 2) + 1);
          u[4] = quant_offset(ph.x, stoch);
          u[5] = quant_offset(ph.y, stoch);
          u[6] = quant_offset(ph.z, stoch);
          u[7] = quant_offset(ph.w, stoch);
        }
      }
      Pack8<T> o, av;
      int cc = c;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int pi = pidx(cc);
        T a = bn_act_value<T>(to_f32(xv.v[j]), p_mean[pi], p_is[pi], p_ga[pi],
                              p_be[pi], do_relu, act_max);
        av.v[j] = a;
        o.v[j] = quant_value<T, STOCH>(a, u[j], min_value, inv_scale, scale,
                                       qmax);
        if (full || e + j < e1) vmax = fmaxf(vmax, to_f32(o.v[j]));
        if (++cc == C) cc = 0;
      }
      T* dst = PAD ? slab + (e - e0) : out + e;
      if (full) {
        *(Pack8<T>*)dst = o;
        *(Pack8<T>*)(act + e) = av;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (e + j < e1) {
            dst[j] = o.v[j];
            act[e + j] = av.v[j];
          }
      }
      c += cstep;
      if (c >= C) c -= C;
    }
    if (PAD) {
      __syncthreads();
      const int total = (int)(r1 - r0) * nchunks;  // 8-channel output chunks
      for (int t = threadIdx.x; t < total; t += kBlock) {
        const int lr = t / nchunks;
        const int base = (t - lr * nchunks) * 8;
        Pack8<T> o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o.v[j] = (base + j < C) ? slab[lr * C + base + j]
                                  : from_f32<T>(0.0f);
        *(Pack8<T>*)(out + (r0 + lr) * (int64_t)C_pad + base) = o;
      }
      __syncthreads();
    }
  }
  // block maximum, then an integer atomicMax on the float's bits: for
  // non-negative floats the integer order is the float order, and a maximum
  // does not depend on the order the blocks arrive in
  vmax = wave_max(vmax);
  if ((threadIdx.x & (WAVE - 1)) == 0) wmax[threadIdx.x / WAVE] = vmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wmax[0];
    for (int w = 1; w < kBlock / WAVE; ++w) m = fmaxf(m, wmax[w]);
    atomicMax(max_bits, __float_as_int(m));
  }
}

struct Shape {
  int C;
  int64_t rows;
};

// x: 4-D channels_last (NCHW logical) or 2-D [rows, C], a 16-bit dtype, on
// the GPU, its data 16-byte aligned; per-channel vectors f32 [C]
Shape check_inputs(const char* fn, const torch::Tensor& x,
                   std::initializer_list<torch::Tensor> per_c) {
  TORCH_CHECK(x.is_cuda(), fn, ": expected a GPU tensor");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 ||
                  x.scalar_type() == torch::kHalf,
              fn, ": 16-bit dtypes only");
  TORCH_CHECK(x.dim() == 4 || x.dim() == 2, fn, ": expected a 4-D or 2-D x");
  Shape s;
  if (x.dim() == 4) {
    TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), fn,
                ": expected channels_last x");
    s.rows = x.size(0) * x.size(2) * x.size(3);
  } else {
    TORCH_CHECK(x.is_contiguous(), fn, ": expected contiguous x");
    s.rows = x.size(0);
  }
  s.C = (int)x.size(1);
  TORCH_CHECK(s.C >= 1 && s.rows >= 1, fn, ": empty input");

  TORCH_CHECK(((uintptr_t)x.data_ptr() & 15) == 0, fn,
              ": x must be 16-byte aligned");
  for (const auto& t : per_c)
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                    t.is_contiguous() && t.numel() == s.C,
                fn, ": per-channel tensors must be contiguous f32 [C] on the GPU");
  return s;
}

}  // namespace

// Returns {act (x's shape and layout), xq_pad [rows, C_pad], max f32 [1]}.
// relu and min_value == 0 are required (the maximum relies on values >= 0);
// C_pad is C (no padding) or a multiple of 8 above it.
std::vector<torch::Tensor> bn_act_quant_fwd(
    torch::Tensor x, torch::Tensor mean, torch::Tensor invstd,
    torch::Tensor gamma, torch::Tensor beta, bool relu, double act_max,
    int64_t num_bits, double min_value, double max_value, double stochastic,
    int64_t seed, int64_t C_pad) {
  const char* fn = "bn_act_quant_fwd";
  Shape s = check_inputs(fn, x, {mean, invstd, gamma, beta});
  TORCH_CHECK(relu && min_value == 0.0, fn,
              ": needs relu and min_value == 0");
  TORCH_CHECK(C_pad == s.C || (C_pad > s.C && (C_pad & 7) == 0), fn,
              ": C_pad must be C or a multiple of 8 above it");
  const bool pad = C_pad != s.C;
  const int C = s.C;
  const int ps = pstride(C);
  // largest slab (a multiple of 8 rows) that fits 48 KB next to the constants
  const size_t par_bytes = ((size_t)4 * ps * sizeof(float) + 15) & ~(size_t)15;
  int slab_rows = 64;
  while (pad && slab_rows > 8 &&
         par_bytes + (size_t)slab_rows * C * 2 > 48 * 1024)
    slab_rows >>= 1;
  const size_t lds = par_bytes + (pad ? (size_t)slab_rows * C * 2 : 0);
  TORCH_CHECK(lds <= 64 * 1024, fn, ": C = ", C, " is too wide");
  auto act = torch::empty_like(x);
  auto out = torch::empty({s.rows, C_pad}, x.options());
  auto maxv = torch::zeros({1}, x.options().dtype(torch::kFloat32));
  float qmax = ::powf(2.0f, (float)num_bits) - 1.0f;
  float scale = std::max(((float)max_value - (float)min_value) / qmax, 1e-6f);
  int64_t nslabs = (s.rows + slab_rows - 1) / slab_rows;
  int blocks = (int)std::min<int64_t>(nslabs, kFwdGridCap);
  auto stream = c10::hip::getCurrentHIPStream();
  NN_DISPATCH(x.scalar_type(), "bn_act_quant_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    if constexpr (sizeof(T) == 2) {
      auto launch = [&](auto kfn, float st) {
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kBlock), lds, stream,
                           (const T*)x.data_ptr(), (T*)act.data_ptr(),
                           (T*)out.data_ptr(),
                           (int*)maxv.data_ptr<float>(),
                           mean.data_ptr<float>(), invstd.data_ptr<float>(),
                           gamma.data_ptr<float>(), beta.data_ptr<float>(),
                           s.rows, C, (int)C_pad, slab_rows, ps, 1,
                           (float)act_max, (float)min_value, 1.0f / scale,
                           scale, qmax, st, (uint64_t)seed, g_seed_base);
      };
      if (stochastic > 0) {
        if (pad) launch(&bn_act_quant_fwd_kernel<T, true, true>, (float)stochastic);
        else launch(&bn_act_quant_fwd_kernel<T, true, false>, (float)stochastic);
      } else {
        if (pad) launch(&bn_act_quant_fwd_kernel<T, false, true>, 0.0f);
        else launch(&bn_act_quant_fwd_kernel<T, false, false>, 0.0f);
      }
    }
  });
  HIP_CHECK_LAST();
  return {act, out, maxv};
}
