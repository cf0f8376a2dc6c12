// The MFMA tile abstraction and the implicit-GEMM geometry shared by the conv
// kernels (conv_mfma.hip) and the crossbar kernels (xbar_*.hip).
//
// A/B/C fragment maps for v_mfma_f32_16x16x32_bf16 (cdna_hip_programming.md
// §3): A[i][k]: i = lane&15, k = 8*(lane>>4)+j (j=0..7, 8 bf16 = 4 VGPRs);
// B[k][j]: j = lane&15, same k split; C/D: col = lane&15,
// row = 4*(lane>>4) + reg.
//
// Everything but check_sigma_mode sits in an unnamed namespace: ConvGeom is a
// kernel parameter, so each translation unit keeps kernels (and helpers) of
// its own, and nothing here is defined twice at link time.
#pragma once

#include <torch/extension.h>
#include <ATen/ATen.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int BM = 64;
constexpr int BN = 64;
constexpr int BK = 32;

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x8 = __attribute__((ext_vector_type(8))) float;

// ---------------------------------------------------------------------------
// Compute-type traits: one MFMA tile abstraction per input dtype.
//   bf16 -> v_mfma_f32_16x16x32_bf16 (8 bf16/lane fragments)
//   fp16 -> v_mfma_f32_16x16x32_f16
//   fp32 -> v_mfma_f32_16x16x4_f32 x8 (EXACT f32 at the f32 vector rate --
//           gfx950 has no xf32; cdna_hip_programming.md §3). The f32 LDS
//           image stores k at permuted position (k&3)*8 + (k>>2) so each
//           lane's 8 needed elements (k = q + 4*kk, q = lane>>4) are the
//           contiguous span [q*8, q*8+8) -> one 32-B read.
// All three share the C/D fragment map (dtype-independent on gfx950), so
// accumulators and epilogues are identical.
// ---------------------------------------------------------------------------

template <typename T> struct Mma;

template <> struct Mma<bf16> {
  using frag = bf16x8;
  static constexpr int STRIDE = 80;   // 32 el * 2 B + 16 B skew
  static DEV_INLINE void store8(char* lds, int row, int k0, const float* v) {
    bf16 tmp[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) tmp[j] = __float2bfloat16(v[j]);
    *(bf16x8*)(lds + row * STRIDE + k0 * 2) = *(bf16x8*)tmp;
  }
  static DEV_INLINE frag load(char* lds, int row, int lane) {
    return *(frag*)(lds + row * STRIDE + (lane >> 4) * 16);
  }
  static DEV_INLINE void mma(const frag& a, const frag& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  static DEV_INLINE void store1(char* lds, int row, int k, float v) {
    *(bf16*)(lds + row * STRIDE + k * 2) = __float2bfloat16(v);
  }
  static DEV_INLINE void store1n(char* lds, int row, int k, bf16 v) {
    *(bf16*)(lds + row * STRIDE + k * 2) = v;
  }
  // read the lane's fragment from a RAW 32-element span (no tile rows)
  static DEV_INLINE frag load_span(const char* base, int lane) {
    return *(frag*)(base + (lane >> 4) * 16);
  }
};

template <> struct Mma<_Float16> {
  using frag = f16x8;
  static constexpr int STRIDE = 80;
  static DEV_INLINE void store8(char* lds, int row, int k0, const float* v) {
    _Float16 tmp[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) tmp[j] = (_Float16)v[j];
    *(f16x8*)(lds + row * STRIDE + k0 * 2) = *(f16x8*)tmp;
  }
  static DEV_INLINE frag load(char* lds, int row, int lane) {
    return *(frag*)(lds + row * STRIDE + (lane >> 4) * 16);
  }
  static DEV_INLINE void mma(const frag& a, const frag& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  }
  static DEV_INLINE void store1(char* lds, int row, int k, float v) {
    *(_Float16*)(lds + row * STRIDE + k * 2) = (_Float16)v;
  }
  static DEV_INLINE void store1n(char* lds, int row, int k, _Float16 v) {
    *(_Float16*)(lds + row * STRIDE + k * 2) = v;
  }
  static DEV_INLINE frag load_span(const char* base, int lane) {
    return *(frag*)(base + (lane >> 4) * 16);
  }
};

template <> struct Mma<float> {
  using frag = f32x8;
  static constexpr int STRIDE = 144;  // 32 el * 4 B + 16 B skew
  static DEV_INLINE void store8(char* lds, int row, int k0, const float* v) {
    float* base = (float*)(lds + row * STRIDE);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int k = k0 + j;
      base[((k & 3) << 3) + (k >> 2)] = v[j];
    }
  }
  static DEV_INLINE frag load(char* lds, int row, int lane) {
    return *(frag*)(lds + row * STRIDE + (lane >> 4) * 32);
  }
  static DEV_INLINE void mma(const frag& a, const frag& b, f32x4& acc) {
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc, 0, 0, 0);
  }
  static DEV_INLINE void store1(char* lds, int row, int k, float v) {
    ((float*)(lds + row * STRIDE))[((k & 3) << 3) + (k >> 2)] = v;
  }
  static DEV_INLINE void store1n(char* lds, int row, int k, float v) {
    store1(lds, row, k, v);
  }
  static DEV_INLINE frag load_span(const char* base, int lane) {
    // raw span is k-linear: gather the lane's strided k = q + 4*kk
    frag f;
    int q = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      f[kk] = ((const float*)base)[q + 4 * kk];
    return f;
  }
};

DEV_INLINE float atomic_max_f32(float* addr, float val) {
  // monotone int mapping for IEEE floats
  int* ia = (int*)addr;
  int old = __float_as_int(val);
  if (val >= 0.0f) {
    return __int_as_float(atomicMax(ia, old));
  }
  return __uint_as_float(atomicMin((unsigned int*)ia, (unsigned int)old));
}

struct ConvGeom {
  int N, H, W, C;      // input
  int K, R, S;         // filter
  int OH, OW;          // output
  int stride, pad;
  int64_t M;           // = N*OH*OW rows of the implicit GEMM
  int flat;            // 1: contraction runs over flattened (r,s,c) in one
                       // K-loop (small-C layers: conv1's C=3 would otherwise
                       // waste 90% of each 32-deep MFMA K-step per tap)
  int Kw;     // rows readable in the weight tensor (host may row-pad)
};

template <typename scalar_t> struct DevT { using type = scalar_t; };
template <> struct DevT<at::BFloat16> { using type = __hip_bfloat16; };
template <> struct DevT<at::Half> { using type = _Float16; };

inline ConvGeom make_geom(int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad) {
  ConvGeom g;
  g.N = N; g.H = H; g.W = W; g.C = C; g.K = K; g.R = R; g.S = S;
  g.Kw = K;  // weight rows staged-safe (== K unless the host row-pads)
  g.stride = stride; g.pad = pad;
  g.OH = (H + 2 * pad - R) / stride + 1;
  g.OW = (W + 2 * pad - S) / stride + 1;
  g.M = (int64_t)N * g.OH * g.OW;
  // flatten the contraction when per-tap C wastes most of a 32-deep K-step
  g.flat = (C < 16 && R * S > 1) ? 1 : 0;
  return g;
}

// Linear layers = the R=S=1, H=W=1 case: a 2-D row-major [B, F] tensor has
// exactly the raw layout of an NHWC (B, F, 1, 1) channels_last tensor
inline ConvGeom linear_geom(const torch::Tensor& x, int64_t out_features) {
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), "linear: 2-D contiguous");
  return make_geom((int)x.size(0), 1, 1, (int)x.size(1), (int)out_features,
                   1, 1, 1, 0);
}

// NHWC raw pointer views of channels_last tensors
inline void check_cl(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, ": expected 4-D channels_last tensor");
}

}  // namespace

// The fused kernels are instantiated for sigma_mode 1 (|w|) and 2
// (|w|^2+|w|); a noise-free mode 0 exists only where allow_zero says so.
// Defined once, in conv_mfma.hip.
void check_sigma_mode(int64_t sigma_mode, bool allow_zero, const char* who);
