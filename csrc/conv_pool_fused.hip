// Small-C image conv fused with its 2x2 max-pool (gfx950 / CDNA4, NHWC).
//
// The first layer of the 4-layer ConvNet is a 5x5 conv over RGB followed by
// a 2x2 max-pool. Run as im2col -> small-K noisy GEMM -> pool (and, in
// backward, un-pool -> pad -> wgrad GEMM) it moves ~38 GB per step at batch
// 32768 although the result only needs the input, the pooled output and the
// 2-bit argmax code. The two kernels here keep everything else on chip:
//
//   conv_pool_fwd_kernel    noisy conv + pool. Derived from
//       conv_fwd_smallk_kernel (conv_mfma.hip): same LDS-resident wq and
//       f(|w_raw|) weight images, same flat (r,s,c) contraction in 32-wide
//       zero-padded chunks, same Philox counter per 4-aligned logical pixel
//       row -- so the un-pooled values are bit-identical -- but the A tile is
//       gathered from LDS-staged NHWC images and the M rows of a tile are
//       ordered so that every lane owns two complete pooling windows.
//   conv_pool_wgrad_kernel  un-pool + wgrad. Both MFMA operands are formed
//       from per-image LDS copies of x, the pooled gradient and the code.
//
// Fragment maps (v_mfma_f32_16x16x32_{bf16,f16}): A[i][k]: i = lane&15,
// k = 8*(lane>>4)+j; B[k][j]: j = lane&15, same k split; C/D: col = lane&15,
// row = 4*(lane>>4)+reg.

#include <torch/extension.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int BM = 64;        // M rows per forward tile (8 pool units)
constexpr int KROWS = 96;     // rows of the LDS weight images
constexpr int STR = 80;       // tile row stride: 32 el * 2 B + 16 B skew
constexpr int kMaxBlocks = 512;   // forward grid cap: 2 blocks/CU, 256 CUs

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <typename T> struct Mma16;
template <> struct Mma16<bf16> {
  using frag = bf16x8;
  static DEV_INLINE void mma(const frag& a, const frag& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
};
template <> struct Mma16<_Float16> {
  using frag = f16x8;
  static DEV_INLINE void mma(const frag& a, const frag& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
  }
};

// 8 x 16-bit elements as one 16-byte value / MFMA fragment (memcpy, not a
// pointer cast: the element and vector types do not alias)
template <typename T>
DEV_INLINE uint4 pack8(const T* v) {
  uint4 r;
  __builtin_memcpy(&r, v, 16);
  return r;
}

template <typename T>
DEV_INLINE typename Mma16<T>::frag to_frag(const T* v) {
  typename Mma16<T>::frag r;
  __builtin_memcpy(&r, v, 16);
  return r;
}

template <typename T>
DEV_INLINE void store8(char* lds, int row, int k0, const float* v) {
  T tmp[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) tmp[j] = from_f32<T>(v[j]);
  *(uint4*)(lds + row * STR + k0 * 2) = pack8(tmp);
}

template <typename T>
DEV_INLINE typename Mma16<T>::frag load_frag(const char* lds, int row,
                                             int lane) {
  return *(const typename Mma16<T>::frag*)(lds + row * STR + (lane >> 4) * 16);
}

// global -> LDS block copy at the widest width the source address and the
// byte count allow (per-image slices of odd-channel tensors are only 4- or
// 8-byte aligned). The branch is block-uniform.
DEV_INLINE void copy_to_lds(char* dst, const char* __restrict__ src,
                            int nbytes) {
  uintptr_t a = (uintptr_t)src | (uintptr_t)nbytes;
  int t = threadIdx.x;
  if ((a & 15) == 0) {
    for (int i = t * 16; i < nbytes; i += kBlock * 16)
      *(uint4*)(dst + i) = *(const uint4*)(src + i);
  } else if ((a & 7) == 0) {
    for (int i = t * 8; i < nbytes; i += kBlock * 8)
      *(uint2*)(dst + i) = *(const uint2*)(src + i);
  } else if ((a & 3) == 0) {
    for (int i = t * 4; i < nbytes; i += kBlock * 4)
      *(uint32_t*)(dst + i) = *(const uint32_t*)(src + i);
  } else {
    for (int i = t; i < nbytes; i += kBlock) dst[i] = src[i];
  }
}

// --------------------------------------------------------------------------
// Forward: out = maxpool2x2(conv(x, wq) [+bias] + N(0, sqrt(factor*sigma))).
//
// Stride 1, pad 0, OH and OW even, OW % 4 == 0. A "unit" is one 4-wide quad
// of output columns in a PAIR of output rows (2j, 2j+1): 8 conv outputs =
// two pooling windows. A 64-row tile carries 8 units: tile row
//     wm*32 + fm*16 + qi*4 + e   <->   unit 8*t + wm*4 + qi,
//                                      output row 2*pj + fm, column 4*qw + e
// so in the 16x16 accumulator layout (row = 4*(lane>>4)+reg) a lane holds
// quad qi = lane>>4 of row 2*pj in acc[0] and of row 2*pj+1 in acc[1]: both
// windows complete, no LDS or cross-lane traffic for the pool. Each quad is
// a 4-aligned run of the row-major pixel index, i.e. exactly one gauss4 draw
// of the un-fused kernel.
//
// A block walks groups of G consecutive images (grid-stride): the G images
// are copied to LDS once and every A tile of the group is gathered from
// there with a per-thread table of (r,s,c) offsets.
// --------------------------------------------------------------------------

template <typename T, int SIGMA_MODE, bool BIAS>
__global__ __launch_bounds__(kBlock)
void conv_pool_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                          const T* __restrict__ wraw,
                          const float* __restrict__ bias,
                          T* __restrict__ out, uint8_t* __restrict__ code,
                          int N, int H, int W, int C, int K, int S, int rsc,
                          int Kc, int OH, int OW, int G,
                          const float* __restrict__ factor_p, uint64_t seed,
                          const int64_t* __restrict__ seed_base) {
  seed = graph_seed(seed_base, seed);
  const float factor = factor_p[0];
  const int CH = Kc >> 5;            // 32-wide contraction chunks (<= 4)

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                              // CH * 64 rows
  char* b_lds = a_lds + (size_t)CH * BM * STR;     // CH * 96 rows (wq)
  char* c_lds = b_lds + (size_t)CH * KROWS * STR;  // CH * 96 rows (sigma w)
  const T* img = (const T*)(c_lds + (size_t)CH * KROWS * STR);  // G images

  const int row = threadIdx.x >> 2;
  const int seg = threadIdx.x & 3;
  const int wid = threadIdx.x / WAVE;
  const int wm = wid >> 1, wn = wid & 1;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nfrag = (K + 15) >> 4;                 // <= 6
  const int nf_w = (nfrag - wn + 1) >> 1;          // fragments of this wave

  // weight images, staged once per block; the host pads rows to 96 and
  // columns to Kc with zeros, so the loads are unconditional
  for (int rb = 0; rb < KROWS; rb += BM) {
    int k = rb + row;
    if (k >= KROWS) continue;
    for (int ch = 0; ch < CH; ++ch) {
      int col0 = ch * 32 + seg * 8;
      const T* pw = wq + (int64_t)k * Kc + col0;
      const T* pr = wraw + (int64_t)k * Kc + col0;
      float vals[8], sv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        vals[j] = to_f32(pw[j]);
        float v = fabsf(to_f32(pr[j]));
        sv[j] = (SIGMA_MODE == 2) ? v * v + v : v;
      }
      store8<T>(b_lds + (size_t)ch * KROWS * STR, k, seg * 8, vals);
      store8<T>(c_lds + (size_t)ch * KROWS * STR, k, seg * 8, sv);
    }
  }

  // this thread stages columns ch*32 + seg*8 + j of tile row `row`: element
  // offset of flat column (r,s,c) from the patch's top-left pixel, -1 in
  // the zero-padded tail
  int koff[4][8];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int kidx = ch * 32 + seg * 8 + j;
      int c = kidx % C;
      int rs = kidx / C;
      int ss = rs % S;
      int rr = rs / S;
      koff[ch][j] = (kidx < rsc) ? (rr * W + ss) * C + c : -1;
    }

  const int PH = OH >> 1, PW = OW >> 1, QW = OW >> 2;
  const int UPI = PH * QW;                         // units per image
  const int HWC = H * W * C;
  const int ngroups = (N + G - 1) / G;
  const int tiles = (G * UPI + 7) >> 3;            // tiles per group
  const T zero = from_f32<T>(0.0f);

  // staging role of this thread within a tile (see the row map above)
  const int s_unit = (row >> 5) * 4 + ((row >> 2) & 3);
  const int s_fm = (row >> 4) & 1;
  const int s_e = row & 3;

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int n0 = grp * G;
    const int gi = min(G, N - n0);                 // images in this group
    __syncthreads();  // weights staged / previous group's gathers done
    copy_to_lds((char*)img, (const char*)(x + (int64_t)n0 * HWC),
                gi * HWC * (int)sizeof(T));
    __syncthreads();

    for (int t = 0; t < tiles; ++t) {
      {
        int ul = t * 8 + s_unit;
        int im = ul / UPI;
        int rem = ul - im * UPI;
        int pj = rem / QW;
        int qw = rem - pj * QW;
        bool valid = im < gi;
        int base = valid
            ? im * HWC + ((2 * pj + s_fm) * W + 4 * qw + s_e) * C : 0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          if (ch >= CH) break;
          T vals[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int off = koff[ch][j];
            T v = img[base + max(off, 0)];
            vals[j] = (valid && off >= 0) ? v : zero;
          }
          *(uint4*)(a_lds + (size_t)ch * BM * STR + row * STR + seg * 16) =
              pack8(vals);
        }
      }
      __syncthreads();

      f32x4 acc[2][3] = {};
      f32x4 sacc[2][3] = {};
      for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
          auto a = load_frag<T>(a_lds + (size_t)ch * BM * STR,
                                wm * 32 + fm * 16 + (lane & 15), lane);
#pragma unroll
          for (int fi = 0; fi < 3; ++fi) {
            if (fi >= nf_w) break;
            int brow = (wn + 2 * fi) * 16 + (lane & 15);
            auto b = load_frag<T>(b_lds + (size_t)ch * KROWS * STR, brow, lane);
            Mma16<T>::mma(a, b, acc[fm][fi]);
            auto c = load_frag<T>(c_lds + (size_t)ch * KROWS * STR, brow, lane);
            Mma16<T>::mma(a, c, sacc[fm][fi]);
          }
        }
      }

      // epilogue: noise on the logical pixel index, round to the storage
      // type, then pool on the ROUNDED values in maxpool2x2_fwd's order
      // (0,0),(0,1),(1,0),(1,1) with strict > -- same ties, same code
      int ul = t * 8 + wm * 4 + (lane >> 4);
      int im = ul / UPI;
      int rem = ul - im * UPI;
      int pj = rem / QW;
      int qw = rem - pj * QW;
      bool uvalid = im < gi;
      int64_t n = n0 + im;
#pragma unroll
      for (int fi = 0; fi < 3; ++fi) {
        if (fi >= nf_w) break;
        int k = (wn + 2 * fi) * 16 + (lane & 15);
        float bv = 0.0f;
        if (BIAS) bv = (k < K) ? bias[k] : 0.0f;
        float vv[2][4];
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
          int64_t mb = (n * OH + 2 * pj + fm) * OW + 4 * qw;
          float g4[4];
          gauss4(seed, (uint64_t)(mb * K + k), g4);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            float y = acc[fm][fi][reg];
            if (BIAS) y += bv;
            float sig = fmaxf(sacc[fm][fi][reg], 0.0f);
            float noise = g4[reg] * sqrtf(factor * sig);
            float v = y + noise;
            vv[fm][reg] = to_f32(from_f32<T>(v));
          }
        }
        if (uvalid && k < K) {
#pragma unroll
          for (int w2 = 0; w2 < 2; ++w2) {
            float m = vv[0][2 * w2];
            int kk = 0;
            if (vv[0][2 * w2 + 1] > m) { m = vv[0][2 * w2 + 1]; kk = 1; }
            if (vv[1][2 * w2] > m) { m = vv[1][2 * w2]; kk = 2; }
            if (vv[1][2 * w2 + 1] > m) { m = vv[1][2 * w2 + 1]; kk = 3; }
            int64_t o = ((n * PH + pj) * PW + 2 * qw + w2) * K + k;
            out[o] = from_f32<T>(m);
            code[o] = (uint8_t)kk;
          }
        }
      }
      __syncthreads();
    }
  }
}

// --------------------------------------------------------------------------
// Backward: dW[k, (r,s,c)] = sum_m gy[m,k] * x[patch(m), r,s,c] where
// gy[m,k] is the pooled gradient if the argmax code selects position m of
// its window and zero otherwise. Neither the full-resolution gradient nor
// the im2col matrix exists in memory.
//
// The summation is arranged to reproduce, bit for bit, what
// maxpool2x2_bwd -> pad_cols8 -> wgrad_mk_kernel -> parts.sum(0) computes
// (conv_wgrad_from_col at M >= 65536): the contraction over the row-major
// pixel index m is cut into the same contiguous slices (one block each), a
// slice is accumulated by the same chain of 16x16x32 MFMAs over ascending
// 32-aligned runs of m with the gradient as the A and the patch as the B
// operand, and the block writes the same [K8, Cp] fp32 slab that the host
// sums the same way. Fixed order, no float atomics.
//
// A 32-run of m may straddle two images, so a block stages GROUPS of GI
// images (GI * OH*OW a multiple of 32) in LDS: x, pooled gradient and code.
// A lane's 8 contraction elements are two 4-aligned quads; per quad the A
// fragment expands 2 pooled (gradient, code) pairs into 4 values and the B
// fragment reads 4 pixels at stride C under the lane's (r,s,c) offset. Each
// wave owns output row-fragments {wave, wave+4} x all JF column fragments and
// walks every run of the slice, so an accumulator sees one sequential chain.
// --------------------------------------------------------------------------

template <typename T, int JF>
__global__ __launch_bounds__(kBlock)
void conv_pool_wgrad_kernel(const T* __restrict__ gp,
                            const uint8_t* __restrict__ code,
                            const T* __restrict__ x,
                            float* __restrict__ parts /* [slices][K8][Cp] */,
                            int N, int H, int W, int C, int K, int K8, int S,
                            int rsc, int Cp, int OH, int OW, int GI,
                            int img_bytes, int g_bytes, int c_bytes,
                            int64_t slice_m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* img_l = smem;
  char* g_l = img_l + (size_t)GI * img_bytes;
  char* c_l = g_l + (size_t)GI * g_bytes;

  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int q = lane >> 4, jl = lane & 15;
  const int PW = OW >> 1, QW = OW >> 2;
  const int NQ = OH * QW;                 // quads per image
  const int OHW = OH * OW;
  const int GIM = GI * OHW;               // pixels per group, % 32 == 0
  const int NRUN = GIM >> 5;              // 32-runs per group
  const int HWC = H * W * C;
  const int PK = (OH >> 1) * PW * K;      // pooled elements per image
  const int KFn = (K8 + 15) >> 4;
  const int nkf = (wid < KFn ? 1 : 0) + (wid + 4 < KFn ? 1 : 0);
  const T zero = from_f32<T>(0.0f);

  int joff[JF];
#pragma unroll
  for (int jf = 0; jf < JF; ++jf) {
    int j = jf * 16 + jl;
    int c = j % C;
    int rs = j / C;
    int ss = rs % S;
    int rr = rs / S;
    joff[jf] = (j < rsc) ? (rr * W + ss) * C + c : -1;
  }

  f32x4 acc[2][JF] = {};

  const int64_t M = (int64_t)N * OHW;
  const int64_t m_start = (int64_t)blockIdx.x * slice_m;   // % 128 == 0
  int64_t m_end = m_start + slice_m;
  if (m_end > M) m_end = M;

  for (int64_t grp = m_start / GIM; grp * GIM < m_end; ++grp) {
    const int64_t n0 = grp * GI;
    const int gi = (int)min((int64_t)GI, (int64_t)N - n0);
    __syncthreads();   // previous group's fragment reads done
    for (int il = 0; il < gi; ++il) {
      copy_to_lds(img_l + (size_t)il * img_bytes,
                  (const char*)(x + (n0 + il) * HWC), HWC * (int)sizeof(T));
      copy_to_lds(g_l + (size_t)il * g_bytes,
                  (const char*)(gp + (n0 + il) * PK), PK * (int)sizeof(T));
      copy_to_lds(c_l + (size_t)il * c_bytes,
                  (const char*)(code + (n0 + il) * PK), PK);
    }
    __syncthreads();

    const int64_t gm0 = grp * GIM;
    const int r_lo = (m_start > gm0) ? (int)((m_start - gm0) >> 5) : 0;
    const int r_hi = (int)min((int64_t)NRUN, (m_end - gm0 + 31) >> 5);
    for (int run = r_lo; run < r_hi; ++run) {
      const T* pimg[2];
      const T* pg[2];
      const uint8_t* pc[2];
      int dsel[2];
      bool qv[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int Ql = run * 8 + 2 * q + h;     // quad within the group
        int il = Ql / NQ;
        int Qi = Ql - il * NQ;
        qv[h] = il < gi;                  // images past N: m >= M, zeros
        if (!qv[h]) { il = 0; Qi = 0; }
        int oh = Qi / QW;
        int ow0 = (Qi - oh * QW) * 4;
        int pin = ((oh >> 1) * PW + (ow0 >> 1)) * K;
        pimg[h] = (const T*)(img_l + (size_t)il * img_bytes) +
                  (oh * W + ow0) * C;
        pg[h] = (const T*)(g_l + (size_t)il * g_bytes) + pin;
        pc[h] = (const uint8_t*)(c_l + (size_t)il * c_bytes) + pin;
        dsel[h] = (oh & 1) * 2;
      }

      typename Mma16<T>::frag a[2], b[JF];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t >= nkf) break;
        int k = (wid + 4 * t) * 16 + jl;
        bool kval = k < K;
        int kc = kval ? k : 0;
        T av[8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int pp = 0; pp < 2; ++pp) {
            T gv = pg[h][pp * K + kc];
            int cd = pc[h][pp * K + kc];
            bool ok = qv[h] && kval;
            av[h * 4 + pp * 2] = (ok && cd == dsel[h]) ? gv : zero;
            av[h * 4 + pp * 2 + 1] = (ok && cd == dsel[h] + 1) ? gv : zero;
          }
        a[t] = to_frag(av);
      }
#pragma unroll
      for (int jf = 0; jf < JF; ++jf) {
        int jo = max(joff[jf], 0);
        T bv[8];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            T v = pimg[h][e * C + jo];
            bv[h * 4 + e] = (qv[h] && joff[jf] >= 0) ? v : zero;
          }
        b[jf] = to_frag(bv);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t >= nkf) break;
#pragma unroll
        for (int jf = 0; jf < JF; ++jf) Mma16<T>::mma(a[t], b[jf], acc[t][jf]);
      }
    }
  }

  float* slab = parts + (int64_t)blockIdx.x * K8 * Cp;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t >= nkf) break;
#pragma unroll
    for (int jf = 0; jf < JF; ++jf)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = (wid + 4 * t) * 16 + 4 * q + reg;
        int j = jf * 16 + jl;
        if (k < K8 && j < Cp) slab[k * Cp + j] = acc[t][jf][reg];
      }
  }
  // columns past the computed fragments are zero-padding of the flat row
  const int tail = Cp - JF * 16;
  if (tail > 0)
    for (int i = threadIdx.x; i < K8 * tail; i += kBlock)
      slab[(i / tail) * Cp + JF * 16 + i % tail] = 0.0f;
}

struct PoolGeom {
  int N, C, H, W, K, R, S, OH, OW, rsc, Kc;
};

PoolGeom pool_geom(const torch::Tensor& x, int64_t K, int64_t R, int64_t S) {
  PoolGeom g;
  g.N = (int)x.size(0); g.C = (int)x.size(1);
  g.H = (int)x.size(2); g.W = (int)x.size(3);
  g.K = (int)K; g.R = (int)R; g.S = (int)S;
  g.OH = g.H - g.R + 1; g.OW = g.W - g.S + 1;
  g.rsc = g.R * g.S * g.C;
  g.Kc = (g.rsc + 31) & ~31;
  return g;
}

constexpr size_t kLdsMax = 160 * 1024;

size_t fwd_lds_bytes(const PoolGeom& g, int G) {
  return (size_t)(g.Kc >> 5) * STR * (BM + 2 * KROWS) +
         (size_t)G * g.H * g.W * g.C * 2;
}

size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// images per wgrad group: smallest count whose pixels fill whole 32-runs
// (OH*OW is a multiple of 8 for eligible shapes, so 1, 2 or 4)
int64_t wgrad_group(int64_t ohw) {
  int64_t gi = 1;
  while ((gi * ohw) & 31) gi *= 2;
  return gi;
}

void check_cl(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous(at::MemoryFormat::ChannelsLast),
              name, ": expected 4-D channels_last tensor");
}

// flat [96, Kc] weight image: raw [K,R,S,C] rows, zero-padded columns/rows
torch::Tensor flat_weight(const torch::Tensor& w, const PoolGeom& g) {
  auto raw = w.permute({0, 2, 3, 1}).reshape({(int64_t)g.K, (int64_t)g.rsc});
  return at::constant_pad_nd(raw, {0, g.Kc - g.rsc, 0, KROWS - g.K}, 0)
      .contiguous();
}

}  // namespace

// Shapes the fused conv+pool pair supports (stride 1, pad 0 implied).
bool conv_pool_eligible(int64_t C, int64_t H, int64_t W, int64_t K, int64_t R,
                        int64_t S, int64_t elem_size) {
  if (elem_size != 2) return false;
  int64_t OH = H - R + 1, OW = W - S + 1;
  if (OH < 2 || OW < 4 || (OH & 1) || (OW & 3)) return false;
  if (R * S * C > 128 || K > 96 || K < 1) return false;
  if ((H * W * C) & 7) return false;   // 16-B image copies in the forward
  int64_t kc = (R * S * C + 31) & ~(int64_t)31;
  int64_t fwd = (kc >> 5) * STR * (BM + 2 * KROWS) + H * W * C * 2;
  int64_t pk = (OH / 2) * (OW / 2) * K;
  int64_t gi = wgrad_group(OH * OW);
  int64_t bwd = gi * (H * W * C * 2 + 16 + pk * 2 + 16 + pk + 16);
  return fwd <= (int64_t)kLdsMax && bwd <= (int64_t)kLdsMax;
}

// Returns {pooled [N,K,OH/2,OW/2] channels_last, code [N,OH/2,OW/2,K] u8},
// bit-identical to maxpool2x2_fwd(conv_fwd_fused(x, ...)[0]) for the same
// seed.
std::vector<torch::Tensor> conv_pool_fwd_fused(torch::Tensor x,
                                               torch::Tensor wq,
                                               torch::Tensor wraw,
                                               torch::Tensor bias,
                                               int64_t sigma_mode,
                                               torch::Tensor factor,
                                               int64_t seed) {
  check_cl(x, "conv_pool_fwd_fused x");
  TORCH_CHECK(sigma_mode == 1 || sigma_mode == 2,
              "conv_pool_fwd_fused: sigma_mode must be 1 or 2");
  auto g = pool_geom(x, wraw.size(0), wraw.size(2), wraw.size(3));
  TORCH_CHECK(wraw.size(1) == g.C && wq.sizes() == wraw.sizes());
  TORCH_CHECK(conv_pool_eligible(g.C, g.H, g.W, g.K, g.R, g.S,
                                 x.element_size()),
              "conv_pool_fwd_fused: shape not eligible");
  int PH = g.OH / 2, PW = g.OW / 2;
  auto wq_flat = flat_weight(wq, g);
  auto wraw_flat = flat_weight(wraw, g);
  auto out = torch::empty({g.N, g.K, PH, PW},
                          x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto code = torch::empty({g.N, PH, PW, g.K}, x.options().dtype(torch::kUInt8));
  bool has_bias = bias.numel() > 0;
  torch::Tensor bias_f;
  if (has_bias) bias_f = bias.to(torch::kFloat32).contiguous();
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();

  // images per group: least tile padding among {1,2,4} that still leaves
  // room for two blocks per CU
  int upi = PH * (g.OW / 4);
  int G = 1;
  double best = 1e9;
  for (int cand : {1, 2, 4}) {
    if (cand > 1 && fwd_lds_bytes(g, cand) > kLdsMax / 2) continue;
    int u = cand * upi;
    double waste = (double)((u + 7) / 8 * 8) / u;
    if (waste < best - 1e-9) { best = waste; G = cand; }
  }
  size_t lds = fwd_lds_bytes(g, G);
  int ngroups = (g.N + G - 1) / G;
  int blocks = std::min(ngroups, kMaxBlocks);
  if (g.N == 0) return {out, code};

  auto run = [&](auto tag) {
    using T = decltype(tag);
    auto stream = c10::hip::getCurrentHIPStream();
    auto launch = [&](auto sm, auto bi) {
      auto* kfn = &conv_pool_fwd_kernel<T, decltype(sm)::value,
                                        decltype(bi)::value>;
      if (lds > 64 * 1024)
        hipFuncSetAttribute((const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
      hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kBlock), lds, stream,
                         (const T*)x.data_ptr(), (const T*)wq_flat.data_ptr(),
                         (const T*)wraw_flat.data_ptr(),
                         has_bias ? bias_f.data_ptr<float>() : nullptr,
                         (T*)out.data_ptr(), code.data_ptr<uint8_t>(), g.N,
                         g.H, g.W, g.C, g.K, g.S, g.rsc, g.Kc, g.OH, g.OW, G,
                         factor_f.data_ptr<float>(), (uint64_t)seed,
                         g_seed_base);
    };
    using TT = std::true_type; using FF = std::false_type;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    if (sigma_mode == 1) { if (has_bias) launch(S1{}, TT{}); else launch(S1{}, FF{}); }
    else { if (has_bias) launch(S2{}, TT{}); else launch(S2{}, FF{}); }
  };
  if (x.scalar_type() == at::kBFloat16) run(bf16{});
  else run(_Float16{});
  HIP_CHECK_LAST();
  return {out, code};
}

// dW [K,C,R,S] channels_last from the POOLED gradient gp [N,K,PH,PW], the
// forward's argmax code and the conv input x.
torch::Tensor conv_pool_wgrad(torch::Tensor gp, torch::Tensor code,
                              torch::Tensor x, int64_t R, int64_t S) {
  check_cl(gp, "conv_pool_wgrad gp");
  check_cl(x, "conv_pool_wgrad x");
  auto g = pool_geom(x, gp.size(1), R, S);
  TORCH_CHECK(conv_pool_eligible(g.C, g.H, g.W, g.K, g.R, g.S,
                                 x.element_size()),
              "conv_pool_wgrad: shape not eligible");
  TORCH_CHECK(gp.scalar_type() == x.scalar_type());
  int PH = g.OH / 2, PW = g.OW / 2;
  TORCH_CHECK(gp.size(0) == g.N && gp.size(2) == PH && gp.size(3) == PW);
  TORCH_CHECK(code.is_contiguous() && code.scalar_type() == torch::kUInt8 &&
              code.numel() == gp.numel());

  // flat-row geometry and contraction slicing of conv_wgrad_from_col ->
  // linear_wgrad (64x64-tile split-M kernel), reproduced exactly
  int K8 = (g.K + 7) & ~7;
  int Cp = ((g.C & 7) == 0) ? g.rsc : g.Kc;
  int64_t M = (int64_t)g.N * g.OH * g.OW;
  int64_t mtotal = std::max<int64_t>(1, (M + 127) / 128);
  int tiles = ((Cp + 63) / 64) * ((K8 + 63) / 64);
  int64_t target_z = std::max<int64_t>(1, 2048 / tiles);
  int64_t chunks = (mtotal + target_z - 1) / target_z;
  int mslices = (int)((mtotal + chunks - 1) / chunks);   // <= 2048 slabs
  int64_t slice_m = chunks * 128;
  auto parts = torch::empty({(int64_t)mslices, (int64_t)K8 * Cp},
                            x.options().dtype(torch::kFloat32));

  int jf = (g.rsc + 15) / 16;
  int JFv = jf <= 2 ? 2 : (jf <= 5 ? 5 : 8);
  int GI = (int)wgrad_group((int64_t)g.OH * g.OW);
  int pk = PH * PW * g.K;
  int img_bytes = (int)round16((size_t)g.H * g.W * g.C * 2);
  int g_bytes = (int)round16((size_t)pk * 2);
  int c_bytes = (int)round16((size_t)pk);
  size_t lds = (size_t)GI * (img_bytes + g_bytes + c_bytes);

  auto run = [&](auto tag) {
    using T = decltype(tag);
    auto stream = c10::hip::getCurrentHIPStream();
    auto launch = [&](auto jfc) {
      auto* kfn = &conv_pool_wgrad_kernel<T, decltype(jfc)::value>;
      if (lds > 64 * 1024)
        hipFuncSetAttribute((const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
      hipLaunchKernelGGL(kfn, dim3(mslices), dim3(kBlock), lds, stream,
                         (const T*)gp.data_ptr(), code.data_ptr<uint8_t>(),
                         (const T*)x.data_ptr(), parts.data_ptr<float>(), g.N,
                         g.H, g.W, g.C, g.K, K8, g.S, g.rsc, Cp, g.OH, g.OW,
                         GI, img_bytes, g_bytes, c_bytes, slice_m);
    };
    if (JFv == 2) launch(std::integral_constant<int, 2>{});
    else if (JFv == 5) launch(std::integral_constant<int, 5>{});
    else launch(std::integral_constant<int, 8>{});
  };
  if (x.scalar_type() == at::kBFloat16) run(bf16{});
  else run(_Float16{});
  HIP_CHECK_LAST();
  // [K8, Cp] -> [K, R*S*C] -> logical [K,C,R,S] channels_last
  auto dw = parts.sum(0).view({(int64_t)K8, (int64_t)Cp})
                .to(x.scalar_type())
                .narrow(0, 0, g.K).narrow(1, 0, g.rsc)
                .view({(int64_t)g.K, (int64_t)g.R, (int64_t)g.S, (int64_t)g.C})
                .permute({0, 3, 1, 2})
                .contiguous(at::MemoryFormat::ChannelsLast);
  return dw;
}
