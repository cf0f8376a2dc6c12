// MFMA implicit-GEMM convolution kernels for gfx950 (CDNA4), NHWC layout.
//
// One kernel family covers conv2d forward (optionally FUSED with the analog
// noise model: a second "sigma" accumulator fed by |W| or |W|^2+|W| tiles
// derived IN-REGISTER from the raw-weight tile, plus in-kernel Philox
// Gaussian sampling -- the reference pays a whole second cuDNN conv +
// curand pass for this, hardware_model.py:49-83), dgrad and wgrad.
// Linear layers are the R=S=1, H=W=1 case (host wrappers reshape).
//
// Structure (v1, correctness-first; tuned against rocprof after):
//   * block = 256 threads = 4 waves in a 2x2 wave grid
//   * tile = 64(M) x 64(N), K-step 32, v_mfma_f32_16x16x32_bf16; the
//     image-patch forward also has layer-fitted one-block-per-image tiles
//     (conv_fwd_patch_tile_kernel, chosen by patch_tile): 4 waves over M x
//     up to 5 N-fragments for plain convs / stride-1 dgrad with K <= 80,
//     with filter rows that fall wholly into the zero padding skipped
//   * K-loop runs over filter taps (r,s) outer, input-channel slices inner,
//     so NHWC staging loads are channel-contiguous (vectorizable) and there
//     is no im2col materialization
//   * LDS tiles use an 80-byte row stride (64 B data + 16 B skew) so
//     ds_read_b128 fragment reads avoid the row-power-of-2 bank pattern
//   * fp32 path uses v_mfma_f32_16x16x4_f32 (exact f32, for unit tests)
//
// The tile abstraction (Mma<T>, with the A/B/C fragment maps) and ConvGeom
// live in mfma_tile.h; the crossbar kernels (xbar_*.hip) share them.

#include <c10/hip/HIPStream.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include "mfma_tile.h"

namespace {

// --------------------------------------------------------------------------
// Staging helpers: global (NHWC) -> LDS tile [rows][BK], bf16, skewed rows.
// Each of the 256 threads owns 8 consecutive k-elements of one row:
//   row = tid >> 2, seg = tid & 3  (4 segs * 8 el * 2B = 64B per row)
// --------------------------------------------------------------------------

// stage activation tile: rows are output pixels m0+row, cols are the
// contraction slice ck+seg*8 .. +8 (input channels of tap (r,s), or the
// flattened (r,s,c) index when g.flat). bf16 inputs with C%8==0 take one
// 16-byte vector load (NHWC rows are then 16B-aligned).
template <typename T>
DEV_INLINE void stage_x_tap(char* lds, const T* __restrict__ x,
                            const ConvGeom g, int64_t m0, int ck, int r, int s) {
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int64_t m = m0 + row;
  float vals[8];
  bool zero = m >= g.M;
  int n = 0, oh = 0, ow = 0;
  if (!zero) {
    int64_t t = m;
    ow = (int)(t % g.OW); t /= g.OW;
    oh = (int)(t % g.OH); t /= g.OH;
    n = (int)t;
  }
  int c0 = ck + seg * 8;
  if (g.flat) {
    if (zero) {
#pragma unroll
      for (int j = 0; j < 8; ++j) vals[j] = 0.0f;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = c0 + j;
        int c = k % g.C;
        int rs = k / g.C;
        int ss = rs % g.S;
        int rr = rs / g.S;
        int ih = oh * g.stride - g.pad + rr;
        int iw = ow * g.stride - g.pad + ss;
        float v = 0.0f;
        if (rr < g.R && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          v = to_f32(x[(((int64_t)n * g.H + ih) * g.W + iw) * g.C + c]);
        vals[j] = v;
      }
    }
    Mma<T>::store8(lds, row, seg * 8, vals);
    return;
  }
  int ih = oh * g.stride - g.pad + r;
  int iw = ow * g.stride - g.pad + s;
  if (!zero && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
    const T* px = x + (((int64_t)n * g.H + ih) * g.W + iw) * g.C;
    if (sizeof(T) == 2 && (g.C & 7) == 0 && c0 + 8 <= g.C) {
      *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) =
          *(const bf16x8*)(px + c0);
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = c0 + j;
      vals[j] = (c < g.C) ? to_f32(px[c]) : 0.0f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) vals[j] = 0.0f;
  }
  Mma<T>::store8(lds, row, seg * 8, vals);
}

// stage weight tile for tap (r,s): rows are output channels n0+row,
// cols are input channels (or the flattened (r,s,c) slice when g.flat --
// the [K,R,S,C] filter is contiguous in exactly that order).
template <typename T, bool ABS_TRANSFORM, int SIGMA_MODE>
DEV_INLINE void stage_w_tap(char* lds, const T* __restrict__ w,
                            const ConvGeom g, int n0, int ck, int r, int s) {
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int k = n0 + row;
  float vals[8];
  int span = g.flat ? g.R * g.S * g.C : g.C;
  if (k < g.Kw) {  // Kw >= K when the host row-pads (e.g. fc weights)
    const T* pw = g.flat ? (w + (int64_t)k * span)
                         : (w + (((int64_t)k * g.R + r) * g.S + s) * g.C);
    int c0 = ck + seg * 8;
    if (sizeof(T) == 2 && c0 + 8 <= span) {
      // one 16-B vector load; the ABS transform runs on registers
      T raw[8];
      *(bf16x8*)raw = *(const bf16x8*)(pw + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = to_f32(raw[j]);
        if (ABS_TRANSFORM) {
          v = fabsf(v);
          if (SIGMA_MODE == 2) v = v * v + v;
        }
        vals[j] = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int c = c0 + j;
        float v = (c < span) ? to_f32(pw[c]) : 0.0f;
        if (ABS_TRANSFORM) {
          v = fabsf(v);
          if (SIGMA_MODE == 2) v = v * v + v;
        }
        vals[j] = v;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) vals[j] = 0.0f;
  }
  Mma<T>::store8(lds, row, seg * 8, vals);
}

// --------------------------------------------------------------------------
// Forward kernel.
// WANT_Y:     accumulate the main output (conv with wq)
// SIGMA_MODE: 0 none, 1 abs(|w|), 2 abs2(|w|^2+|w|)  (uses w_raw tiles)
// TELEM:      also accumulate sum(sigma_abs), sum|noise|, max(y_clean)
//             (when SIGMA_MODE==2 an extra |w| accumulator is carried)
// BIAS:       add bias[n]
// --------------------------------------------------------------------------

template <typename T, bool WANT_Y, int SIGMA_MODE, bool TELEM, bool BIAS>
__global__ __launch_bounds__(kBlock)
void conv_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                     const T* __restrict__ wraw, const float* __restrict__ bias,
                     T* __restrict__ out, ConvGeom g,
                     const float* __restrict__ factor_p,
                     uint64_t seed, float* __restrict__ telem /* [3] */,
                     const int64_t* __restrict__ seed_base = nullptr) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  // grid: x = n-tiles, y = m-tiles
  int n0 = blockIdx.x * BN;
  int64_t m0 = (int64_t)blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                                   // BM rows
  char* b_lds = smem + BM * STR;                        // BN rows (wq or wraw)
  char* c_lds = smem + (BM + BN) * STR;                 // BN rows (wraw sigma)
  char* d_lds = smem + (BM + 2 * BN) * STR;             // BN rows (|w| telem)

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  f32x4 acc[2][2] = {};     // y
  f32x4 sacc[2][2] = {};    // sigma (mode 1 or 2)
  f32x4 tacc[2][2] = {};    // sigma_abs for telemetry when mode==2

  const int Rl = g.flat ? 1 : g.R;
  const int Sl = g.flat ? 1 : g.S;
  const int Cl = g.flat ? g.R * g.S * g.C : g.C;
  for (int r = 0; r < Rl; ++r) {
    for (int s = 0; s < Sl; ++s) {
      for (int ck = 0; ck < Cl; ck += BK) {
        stage_x_tap(a_lds, x, g, m0, ck, r, s);
        if (WANT_Y) stage_w_tap<T, false, 0>(b_lds, wq, g, n0, ck, r, s);
        if (SIGMA_MODE > 0)
          stage_w_tap<T, true, SIGMA_MODE>(c_lds, wraw, g, n0, ck, r, s);
        if (TELEM && SIGMA_MODE == 2)
          stage_w_tap<T, true, 1>(d_lds, wraw, g, n0, ck, r, s);
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
          auto a = Mma<T>::load(a_lds, wm * 32 + fm * 16 + (lane & 15), lane);
#pragma unroll
          for (int fn = 0; fn < 2; ++fn) {
            int brow = wn * 32 + fn * 16 + (lane & 15);
            if (WANT_Y) {
              auto b = Mma<T>::load(b_lds, brow, lane);
              Mma<T>::mma(a, b, acc[fm][fn]);
            }
            if (SIGMA_MODE > 0) {
              auto bs = Mma<T>::load(c_lds, brow, lane);
              Mma<T>::mma(a, bs, sacc[fm][fn]);
            }
            if (TELEM && SIGMA_MODE == 2) {
              auto bt = Mma<T>::load(d_lds, brow, lane);
              Mma<T>::mma(a, bt, tacc[fm][fn]);
            }
          }
        }
        __syncthreads();
      }
    }
  }

  // epilogue: bias, noise, stores (+ telemetry reductions)
  float t_sum_sigma = 0.0f, t_sum_noise = 0.0f, t_max_y = -INFINITY;
#pragma unroll
  for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
      int64_t mb = m0 + wm * 32 + fm * 16 + 4 * (lane >> 4);
      int n = n0 + wn * 32 + fn * 16 + (lane & 15);
      float g4[4];
      if (SIGMA_MODE > 0) gauss4(seed, (uint64_t)(mb * g.K + n), g4);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int64_t m = mb + reg;
        if (m < g.M && n < g.K) {
          float y = WANT_Y ? acc[fm][fn][reg] : 0.0f;
          if (BIAS) y += bias[n];
          float v = y;
          if (SIGMA_MODE > 0) {
            float sig = fmaxf(sacc[fm][fn][reg], 0.0f);
            float noise = g4[reg] * sqrtf(factor * sig);
            v = y + noise;
            if (TELEM) {
              t_sum_noise += fabsf(noise);
              t_max_y = fmaxf(t_max_y, y);
              t_sum_sigma += (SIGMA_MODE == 2) ? tacc[fm][fn][reg]
                                               : sacc[fm][fn][reg];
            }
          }
          out[m * g.K + n] = from_f32<T>(v);
        }
      }
    }
  }
  if (TELEM && SIGMA_MODE > 0) {
    __shared__ float red[4];
    float s0 = block_sum(t_sum_sigma, red);
    __syncthreads();
    float s1 = block_sum(t_sum_noise, red);
    __syncthreads();
    // block max via wave max + lds
    float m0v = wave_max(t_max_y);
    __shared__ float redm[4];
    if ((threadIdx.x & (WAVE - 1)) == 0) redm[threadIdx.x / WAVE] = m0v;
    __syncthreads();
    if (threadIdx.x == 0) {
      atomicAdd(&telem[0], s0);
      atomicAdd(&telem[1], s1);
      float mm = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
      atomic_max_f32(&telem[2], mm);
    }
  }
}

// --------------------------------------------------------------------------
// Small-K fused GEMM: out[M, K] = x2[M, Kc] @ w[K, Kc]^T (+sigma +noise),
// for Kc <= 128 (contraction fits LDS whole) and K <= 96 (one block tile
// covers every output channel). This is the conv1-as-im2col shape
// ([1.6M, 80] @ [65, 80]^T at batch 2048): the generic kernel pays a
// sync per 32-deep k-step and re-reads the A rows once per 32-wide
// n-tile; here the whole weight set is staged ONCE per block (it stays
// LDS-resident across the block's grid-stride m-tiles) and each A tile
// is read exactly once, giving one global pass over x2.
// Wave layout: 4 waves, wm = wave>>1 covers m 0..63, wn = wave&1 owns
// output fragments f in {wn, wn+2, wn+4} (16 channels each, K<=96).
// 16-bit dtypes only (fp32 LDS image would not fit).
// --------------------------------------------------------------------------

template <typename T, bool WANT_Y, int SIGMA_MODE, bool TELEM, bool BIAS>
__global__ __launch_bounds__(kBlock)
void conv_fwd_smallk_kernel(const T* __restrict__ x2, const T* __restrict__ wq,
                            const T* __restrict__ wraw,
                            const float* __restrict__ bias,
                            T* __restrict__ out, int64_t M, int K, int Kc,
                            const float* __restrict__ factor_p, uint64_t seed,
                            float* __restrict__ telem,
                            const int64_t* __restrict__ seed_base = nullptr) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  constexpr int STR = Mma<T>::STRIDE;
  const int CH = (Kc + 31) >> 5;     // 32-wide contraction chunks (<= 4),
                                     // last one zero-padded when Kc % 32
  const int KROWS = 96;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                              // CH * 64 rows
  char* b_lds = smem + (size_t)CH * BM * STR;      // CH * 96 rows (wq)
  char* c_lds = b_lds + (size_t)CH * KROWS * STR;  // CH * 96 rows (sigma w)
  char* d_lds = c_lds + (size_t)CH * KROWS * STR;  // CH * 96 rows (|w|)

  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  const int nfrag = (K + 15) >> 4;                 // <= 6
  const int nf_w = (nfrag - wn + 1) >> 1;          // fragments of this wave

  // stage the full weight set once; the host pads rows to 96 and columns
  // to round32(Kc) with zeros, so the loads are unconditional
  for (int rb = 0; rb < KROWS; rb += BM) {
    int k = rb + row;
    if (k >= KROWS) continue;  // rows 96..127 of the second pass
    for (int ch = 0; ch < CH; ++ch) {
      int col0 = ch * 32 + seg * 8;
      float vals[8];
      const T* pw = wq + (int64_t)k * Kc + col0;
      const T* pr = wraw + (int64_t)k * Kc + col0;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vals[j] = WANT_Y ? to_f32(pw[j]) : 0.0f;
      if (WANT_Y)
        Mma<T>::store8(b_lds + (size_t)ch * KROWS * STR, k, seg * 8, vals);
      if (SIGMA_MODE > 0) {
        float sv[8], tv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = fabsf(to_f32(pr[j]));
          tv[j] = v;
          sv[j] = (SIGMA_MODE == 2) ? v * v + v : v;
        }
        Mma<T>::store8(c_lds + (size_t)ch * KROWS * STR, k, seg * 8, sv);
        if (TELEM && SIGMA_MODE == 2)
          Mma<T>::store8(d_lds + (size_t)ch * KROWS * STR, k, seg * 8, tv);
      }
    }
  }
  __syncthreads();

  float t_sum_sigma = 0.0f, t_sum_noise = 0.0f, t_max_y = -INFINITY;
  int64_t mtiles = (M + BM - 1) / BM;

  // A tiles are register-prefetched: the next tile's global loads issue
  // during the current tile's MFMA+epilogue (PMC: 41% of wave-cycles
  // were parked on the synchronous A-load at 2 blocks/CU)
  T areg[4][8];
  auto load_a = [&](int64_t mt_) {
    int64_t m = mt_ * BM + row;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch >= CH) break;
      int col0 = ch * 32 + seg * 8;
      if (m < M && sizeof(T) == 2) {  // Kc is round32: no column tail
        *(bf16x8*)areg[ch] = *(const bf16x8*)(x2 + m * Kc + col0);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          areg[ch][j] = (m < M && col0 + j < Kc)
                            ? x2[m * Kc + col0 + j] : from_f32<T>(0.0f);
      }
    }
  };
  if (blockIdx.x < mtiles) load_a(blockIdx.x);

  for (int64_t mt = blockIdx.x; mt < mtiles; mt += gridDim.x) {
    int64_t m0 = mt * BM;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      if (ch >= CH) break;
      if (sizeof(T) == 2) {
        *(bf16x8*)(a_lds + (size_t)ch * BM * STR + row * STR + seg * 16) =
            *(bf16x8*)areg[ch];
      } else {
        float vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = to_f32(areg[ch][j]);
        Mma<T>::store8(a_lds + (size_t)ch * BM * STR, row, seg * 8, vals);
      }
    }
    __syncthreads();
    if (mt + gridDim.x < mtiles) load_a(mt + gridDim.x);

    f32x4 acc[2][3] = {};
    f32x4 sacc[2][3] = {};
    f32x4 tacc[2][3] = {};
    for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
        auto a = Mma<T>::load(a_lds + (size_t)ch * BM * STR,
                              wm * 32 + fm * 16 + (lane & 15), lane);
#pragma unroll
        for (int fi = 0; fi < 3; ++fi) {
          if (fi >= nf_w) break;  // constant-trip unroll, predicated tail
          int brow = (wn + 2 * fi) * 16 + (lane & 15);
          if (WANT_Y) {
            auto b = Mma<T>::load(b_lds + (size_t)ch * KROWS * STR, brow, lane);
            Mma<T>::mma(a, b, acc[fm][fi]);
          }
          if (SIGMA_MODE > 0) {
            auto c = Mma<T>::load(c_lds + (size_t)ch * KROWS * STR, brow, lane);
            Mma<T>::mma(a, c, sacc[fm][fi]);
          }
          if (TELEM && SIGMA_MODE == 2) {
            auto d = Mma<T>::load(d_lds + (size_t)ch * KROWS * STR, brow, lane);
            Mma<T>::mma(a, d, tacc[fm][fi]);
          }
        }
      }
    }

    // epilogue
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
      for (int fi = 0; fi < 3; ++fi) {
        if (fi >= nf_w) break;
        int64_t mb = m0 + wm * 32 + fm * 16 + 4 * (lane >> 4);
        int k = (wn + 2 * fi) * 16 + (lane & 15);
        float g4[4];
        if (SIGMA_MODE > 0) gauss4(seed, (uint64_t)(mb * K + k), g4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          int64_t m = mb + reg;
          if (m < M && k < K) {
            float y = WANT_Y ? acc[fm][fi][reg] : 0.0f;
            if (BIAS) y += bias[k];
            float v = y;
            if (SIGMA_MODE > 0) {
              float sig = fmaxf(sacc[fm][fi][reg], 0.0f);
              float noise = g4[reg] * sqrtf(factor * sig);
              v = y + noise;
              if (TELEM) {
                t_sum_noise += fabsf(noise);
                t_max_y = fmaxf(t_max_y, y);
                t_sum_sigma += (SIGMA_MODE == 2) ? tacc[fm][fi][reg]
                                                 : sacc[fm][fi][reg];
              }
            }
            out[m * K + k] = from_f32<T>(v);
          }
        }
      }
    }
    __syncthreads();
  }

  if (TELEM && SIGMA_MODE > 0) {
    __shared__ float red[4];
    float s0 = block_sum(t_sum_sigma, red);
    __syncthreads();
    float s1 = block_sum(t_sum_noise, red);
    __syncthreads();
    float m0v = wave_max(t_max_y);
    __shared__ float redm[4];
    if ((threadIdx.x & (WAVE - 1)) == 0) redm[threadIdx.x / WAVE] = m0v;
    __syncthreads();
    if (threadIdx.x == 0) {
      atomicAdd(&telem[0], s0);
      atomicAdd(&telem[1], s1);
      atomic_max_f32(&telem[2],
                     fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3])));
    }
  }
}

// --------------------------------------------------------------------------
// Dgrad: dx[n,ih,iw,c] = sum_{r,s,k} g[n,oh,ow,k] * w[k,r,s,c]
// with oh = (ih + pad - r)/stride when divisible. Implicit GEMM over taps:
// A rows = input pixels, contraction = output channels K, B = wt[r,s,c,k]
// ([R*S*C, K] row-major: contraction contiguous).
// --------------------------------------------------------------------------

template <typename T>
DEV_INLINE void stage_g_tap_dgrad(char* lds, const T* __restrict__ gy,
                                  const ConvGeom g, int64_t m0, int kk, int r,
                                  int s) {
  // rows = input pixels (n, ih, iw); cols = output channels kk+seg*8..
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int64_t m = m0 + row;
  int64_t MI = (int64_t)g.N * g.H * g.W;
  float vals[8];
  bool ok = false;
  const T* pg = nullptr;
  if (m < MI) {
    int64_t t = m;
    int iw = (int)(t % g.W); t /= g.W;
    int ih = (int)(t % g.H); t /= g.H;
    int n = (int)t;
    int ohs = ih + g.pad - r;
    int ows = iw + g.pad - s;
    if (ohs >= 0 && ows >= 0 && ohs % g.stride == 0 && ows % g.stride == 0) {
      int oh = ohs / g.stride, ow = ows / g.stride;
      if (oh < g.OH && ow < g.OW) {
        pg = gy + (((int64_t)n * g.OH + oh) * g.OW + ow) * g.K;
        ok = true;
      }
    }
  }
  int k0 = kk + seg * 8;
  if (ok && sizeof(T) == 2 && (g.K & 7) == 0 && k0 + 8 <= g.K) {
    *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) =
        *(const bf16x8*)(pg + k0);
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int k = k0 + j;
    vals[j] = (ok && k < g.K) ? to_f32(pg[k]) : 0.0f;
  }
  Mma<T>::store8(lds, row, seg * 8, vals);
}

template <typename T>
DEV_INLINE void stage_wt_tap(char* lds, const T* __restrict__ wt,
                             const ConvGeom g, int n0, int kk, int r, int s) {
  // wt layout [R, S, C, K]; rows = input channels n0+row, cols = K
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int c = n0 + row;
  float vals[8];
  if (c < g.C) {
    const T* pw = wt + (((int64_t)r * g.S + s) * g.C + c) * g.K;
    int k0 = kk + seg * 8;
    if (sizeof(T) == 2 && (g.K & 7) == 0 && k0 + 8 <= g.K) {
      *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) =
          *(const bf16x8*)(pw + k0);
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int k = k0 + j;
      vals[j] = (k < g.K) ? to_f32(pw[k]) : 0.0f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) vals[j] = 0.0f;
  }
  Mma<T>::store8(lds, row, seg * 8, vals);
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void conv_dgrad_kernel(const T* __restrict__ gy, const T* __restrict__ wt,
                       T* __restrict__ dx, ConvGeom g) {
  int n0 = blockIdx.x * BN;  // over input channels C
  int64_t m0 = (int64_t)blockIdx.y * BM;  // over input pixels
  int64_t MI = (int64_t)g.N * g.H * g.W;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;
  char* b_lds = smem + BM * STR;

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  f32x4 acc[2][2] = {};

  for (int r = 0; r < g.R; ++r) {
    for (int s = 0; s < g.S; ++s) {
      for (int kk = 0; kk < g.K; kk += BK) {
        stage_g_tap_dgrad(a_lds, gy, g, m0, kk, r, s);
        stage_wt_tap(b_lds, wt, g, n0, kk, r, s);
        __syncthreads();
#pragma unroll
        for (int fm = 0; fm < 2; ++fm) {
          auto a = Mma<T>::load(a_lds, wm * 32 + fm * 16 + (lane & 15), lane);
#pragma unroll
          for (int fn = 0; fn < 2; ++fn) {
            auto b = Mma<T>::load(b_lds, wn * 32 + fn * 16 + (lane & 15), lane);
            Mma<T>::mma(a, b, acc[fm][fn]);
          }
        }
        __syncthreads();
      }
    }
  }

#pragma unroll
  for (int fm = 0; fm < 2; ++fm)
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int64_t m = m0 + wm * 32 + fm * 16 + 4 * (lane >> 4) + reg;
        int c = n0 + wn * 32 + fn * 16 + (lane & 15);
        if (m < MI && c < g.C) dx[m * g.C + c] = from_f32<T>(acc[fm][fn][reg]);
      }
}

// --------------------------------------------------------------------------
// Wgrad: dw[k,r,s,c] = sum_{n,oh,ow} g[n,oh,ow,k] * x[n,ih,iw,c].
// Contraction over output pixels (huge): each block owns (tap, k-tile,
// c-tile) and a grid-z slice of the M range; partials atomicAdd into an
// f32 buffer. Staging transposes G and X into LDS so fragments read
// contraction-contiguous.
// --------------------------------------------------------------------------

template <typename T>
DEV_INLINE void stage_gx_transposed(char* g_lds, char* x_lds,
                                    const T* __restrict__ gy,
                                    const T* __restrict__ x, const ConvGeom g,
                                    int64_t m0, int k0, int c0, int r, int s) {
  // 256 threads load a [BK=32 m] x [64 col] slab of G and X each, writing
  // transposed into LDS rows [col][m] through the compute-type store
  // (which also applies the f32 k-permutation). Thread: mi = tid&31,
  // colseg = tid>>5 (8 segs of 8 cols).
  int mi = threadIdx.x & 31;
  int colseg = threadIdx.x >> 5;
  int64_t m = m0 + mi;
  bool mok = m < g.M;
  int n = 0, ih = 0, iw = 0;
  const T* px = nullptr;
  const T* pg = nullptr;
  if (mok) {
    int64_t t = m;
    int ow = (int)(t % g.OW); t /= g.OW;
    int oh = (int)(t % g.OH); t /= g.OH;
    n = (int)t;
    ih = oh * g.stride - g.pad + r;
    iw = ow * g.stride - g.pad + s;
    pg = gy + (((int64_t)n * g.OH + oh) * g.OW + ow) * g.K;
    if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
      px = x + (((int64_t)n * g.H + ih) * g.W + iw) * g.C;
  }
  if (g.flat) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int kcol = k0 + colseg * 8 + j;
      float gv = (mok && kcol < g.K) ? to_f32(pg[kcol]) : 0.0f;
      Mma<T>::store1(g_lds, colseg * 8 + j, mi, gv);
      // flat column -> (r', s', c) decoded per element
      int fcol = c0 + colseg * 8 + j;
      float xv = 0.0f;
      if (mok && fcol < g.R * g.S * g.C) {
        int c = fcol % g.C;
        int rs = fcol / g.C;
        int ss = rs % g.S;
        int rr = rs / g.S;
        int t2 = m % ((int64_t)g.OH * g.OW);
        int ow2 = (int)(t2 % g.OW);
        int oh2 = (int)(t2 / g.OW);
        int ih2 = oh2 * g.stride - g.pad + rr;
        int iw2 = ow2 * g.stride - g.pad + ss;
        if (ih2 >= 0 && ih2 < g.H && iw2 >= 0 && iw2 < g.W)
          xv = to_f32(x[(((int64_t)n * g.H + ih2) * g.W + iw2) * g.C + c]);
      }
      Mma<T>::store1(x_lds, colseg * 8 + j, mi, xv);
    }
    return;
  }
  // Keep the values in the NATIVE element type: for 16-bit dtypes the
  // aligned case is one 16-B global vector load per operand (this kernel is
  // global-load bound -- 8 scalar u16 loads here cost ~2.5x on the bench).
  T gvals[8], xvals[8];
  int kc0 = k0 + colseg * 8;
  if (mok && sizeof(T) == 2 && (g.K & 7) == 0 && kc0 + 8 <= g.K) {
    *(bf16x8*)gvals = *(const bf16x8*)(pg + kc0);  // raw 16-B copy (punned)
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int kcol = kc0 + j;
      gvals[j] = (mok && kcol < g.K) ? pg[kcol] : from_f32<T>(0.0f);
    }
  }
  int cc0 = c0 + colseg * 8;
  if (px != nullptr && sizeof(T) == 2 && (g.C & 7) == 0 && cc0 + 8 <= g.C) {
    *(bf16x8*)xvals = *(const bf16x8*)(px + cc0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int ccol = cc0 + j;
      xvals[j] = (px != nullptr && ccol < g.C) ? px[ccol] : from_f32<T>(0.0f);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    Mma<T>::store1n(g_lds, colseg * 8 + j, mi, gvals[j]);
    Mma<T>::store1n(x_lds, colseg * 8 + j, mi, xvals[j]);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void conv_wgrad_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                       float* __restrict__ dw /* [mslices][K,R,S,C] f32 */,
                       ConvGeom g, int mchunks_per_block, int64_t wspan) {
  // grid: x = c-tiles (or flat rsc-tiles), y = k-tiles, z = taps * m-slices
  int taps = g.flat ? 1 : g.R * g.S;
  int tap = blockIdx.z % taps;
  int mslice = blockIdx.z / taps;
  int r = tap / g.S, s = tap % g.S;
  int c0 = blockIdx.x * BN;
  int k0 = blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* g_lds = smem;                        // [64 k rows][32 m]
  char* x_lds = smem + BM * STR;             // [64 c rows][32 m]

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  f32x4 acc[2][2] = {};

  int64_t m_start = (int64_t)mslice * mchunks_per_block * BK;
  int64_t m_end = m_start + (int64_t)mchunks_per_block * BK;
  if (m_end > g.M) m_end = g.M;

  for (int64_t m0 = m_start; m0 < m_end; m0 += BK) {
    stage_gx_transposed(g_lds, x_lds, gy, x, g, m0, k0, c0, r, s);
    __syncthreads();
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      auto a = Mma<T>::load(g_lds, wm * 32 + fm * 16 + (lane & 15), lane);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        auto b = Mma<T>::load(x_lds, wn * 32 + fn * 16 + (lane & 15), lane);
        Mma<T>::mma(a, b, acc[fm][fn]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int fm = 0; fm < 2; ++fm)
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = k0 + wm * 32 + fm * 16 + 4 * (lane >> 4) + reg;
        int c = c0 + wn * 32 + fn * 16 + (lane & 15);
        int span = g.flat ? g.R * g.S * g.C : g.C;
        if (k < g.K && c < span) {
          int64_t off = g.flat
              ? (int64_t)k * span + c
              : (((int64_t)k * g.R + r) * g.S + s) * g.C + c;
          // one writer per (mslice, k, tap, c): plain store into this
          // m-slice's partial image; the host sums partials in fixed
          // order (deterministic, no atomic race ordering)
          dw[(int64_t)mslice * wspan + off] = acc[fm][fn][reg];
        }
      }
}

// --------------------------------------------------------------------------
// Fast GEMM wgrad for the flat/linear case: dw[K, C] += gy[M, K]^T @ x[M, C]
// with K % 8 == 0, C % 8 == 0, 16-bit dtype. 128-deep contraction rounds
// (4x fewer barriers than the generic kernel), 16-B vector global loads,
// and a register pipeline that loads round i+1 while round i's MFMAs run.
// LDS images are [64 rows][128 m] at a 272-B row stride (16-B skew).
// --------------------------------------------------------------------------

constexpr int WG_BK = 128;          // contraction (m) depth per round
constexpr int WG_LSTR = WG_BK * 2 + 16;

template <typename T>
DEV_INLINE void wgrad_mk_load(T dst[4][8], const T* __restrict__ src,
                              int64_t m0, int64_t M, int cols, int c0) {
  // thread t covers 4 (m_i, seg) slots: idx = t + i*256, m_i = idx>>3,
  // seg = idx&7 (64 cols = 8 segs of 8)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int idx = threadIdx.x + i * kBlock;
    int mi = idx >> 3;
    int seg = idx & 7;
    int64_t m = m0 + mi;
    int c = c0 + seg * 8;
    if (m < M && c + 8 <= cols) {
      *(bf16x8*)dst[i] = *(const bf16x8*)(src + m * cols + c);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[i][j] = from_f32<T>(0.0f);
    }
  }
}

// The transposed scatter writes 16 rows at stride 8 per instruction; at a
// 272-B row stride those land in only 2 LDS banks (8-way conflict). A
// row-dependent 16-B chunk rotation spreads them; fragment reads apply
// the same rotation (still one aligned b128 per fragment).
DEV_INLINE int wg_swz(int row, int chunk) { return ((chunk + (row >> 3)) & 15); }

template <typename T>
DEV_INLINE void wgrad_mk_store(char* lds, const T src[4][8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int idx = threadIdx.x + i * kBlock;
    int mi = idx >> 3;
    int seg = idx & 7;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = seg * 8 + j;
      *(T*)(lds + row * WG_LSTR + wg_swz(row, mi >> 3) * 16 + (mi & 7) * 2) =
          src[i][j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void wgrad_mk_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                     float* __restrict__ dw /* [K, C] f32 */, int64_t M,
                     int K, int C, int mchunks_per_block) {
  int c0 = blockIdx.x * BN;
  int k0 = blockIdx.y * BM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* g_lds = smem;                      // [64 k rows][128 m]
  char* x_lds = smem + BM * WG_LSTR;       // [64 c rows][128 m]

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  f32x4 acc[2][2] = {};

  int64_t m_start = (int64_t)blockIdx.z * mchunks_per_block * WG_BK;
  int64_t m_end = m_start + (int64_t)mchunks_per_block * WG_BK;
  if (m_end > M) m_end = M;

  T greg[4][8], xreg[4][8];
  if (m_start < m_end) {
    wgrad_mk_load(greg, gy, m_start, M, K, k0);
    wgrad_mk_load(xreg, x, m_start, M, C, c0);
  }

  for (int64_t m0 = m_start; m0 < m_end; m0 += WG_BK) {
    wgrad_mk_store(g_lds, greg);
    wgrad_mk_store(x_lds, xreg);
    __syncthreads();
    if (m0 + WG_BK < m_end) {
      wgrad_mk_load(greg, gy, m0 + WG_BK, M, K, k0);
      wgrad_mk_load(xreg, x, m0 + WG_BK, M, C, c0);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
        int arow = wm * 32 + fm * 16 + (lane & 15);
        auto a = *(typename Mma<T>::frag*)(
            g_lds + arow * WG_LSTR +
            wg_swz(arow, ks * 4 + (lane >> 4)) * 16);
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          int brow = wn * 32 + fn * 16 + (lane & 15);
          auto b = *(typename Mma<T>::frag*)(
              x_lds + brow * WG_LSTR +
              wg_swz(brow, ks * 4 + (lane >> 4)) * 16);
          Mma<T>::mma(a, b, acc[fm][fn]);
        }
      }
    }
    __syncthreads();
  }

  // each (ctile, ktile, z) block owns a disjoint region of its z-slice:
  // plain stores into per-slice partials (summed host-side). The atomic
  // version serialized ~90 contenders per output word on wide shapes.
  float* slab = dw + (int64_t)blockIdx.z * K * C;
#pragma unroll
  for (int fm = 0; fm < 2; ++fm)
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = k0 + wm * 32 + fm * 16 + 4 * (lane >> 4) + reg;
        int c = c0 + wn * 32 + fn * 16 + (lane & 15);
        if (k < K && c < C) slab[(int64_t)k * C + c] = acc[fm][fn][reg];
      }
}

// 128x128-tile variant for wide outputs (e.g. conv2 wgrad: K=120,
// C=3000): the 64-wide c-tiles of wgrad_mk_kernel re-read the small gy
// operand once per tile (47x = 2.3 GB at batch 2048); doubling both
// tile sides quarters the cross-reads. No register prefetch (the tile
// needs 8 staging slots per thread per tensor; the extra 64 VGPRs would
// cost a wave); 4 waves as 2x2 quadrants of 64x64, acc[4][4].
template <typename T>
DEV_INLINE void wgrad_mk4_stage(char* lds, const T* __restrict__ src,
                                int64_t m0, int64_t M, int cols, int c0) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int idx = threadIdx.x + i * kBlock;  // 0..2047
    int mi = idx >> 4;                   // 0..127 (m)
    int seg = idx & 15;                  // 0..15  (8-col group)
    int64_t m = m0 + mi;
    int c = c0 + seg * 8;
    T vals[8];
    if (m < M && c + 8 <= cols) {
      *(bf16x8*)vals = *(const bf16x8*)(src + m * cols + c);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) vals[j] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = seg * 8 + j;
      *(T*)(lds + row * WG_LSTR + wg_swz(row, mi >> 3) * 16 + (mi & 7) * 2) =
          vals[j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void wgrad_mk4_kernel(const T* __restrict__ gy, const T* __restrict__ x,
                      float* __restrict__ dw /* [K, C] f32 */, int64_t M,
                      int K, int C, int mchunks_per_block) {
  int c0 = blockIdx.x * 128;
  int k0 = blockIdx.y * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* g_lds = smem;                        // [128 k rows][128 m]
  char* x_lds = smem + 128 * WG_LSTR;        // [128 c rows][128 m]

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  f32x4 acc[4][4] = {};

  int64_t m_start = (int64_t)blockIdx.z * mchunks_per_block * WG_BK;
  int64_t m_end = m_start + (int64_t)mchunks_per_block * WG_BK;
  if (m_end > M) m_end = M;

  for (int64_t m0 = m_start; m0 < m_end; m0 += WG_BK) {
    wgrad_mk4_stage(g_lds, gy, m0, M, K, k0);
    wgrad_mk4_stage(x_lds, x, m0, M, C, c0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int fm = 0; fm < 4; ++fm) {
        int arow = wm * 64 + fm * 16 + (lane & 15);
        auto a = *(typename Mma<T>::frag*)(
            g_lds + arow * WG_LSTR +
            wg_swz(arow, ks * 4 + (lane >> 4)) * 16);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
          int brow = wn * 64 + fn * 16 + (lane & 15);
          auto b = *(typename Mma<T>::frag*)(
              x_lds + brow * WG_LSTR +
              wg_swz(brow, ks * 4 + (lane >> 4)) * 16);
          Mma<T>::mma(a, b, acc[fm][fn]);
        }
      }
    }
    __syncthreads();
  }

  float* slab = dw + (int64_t)blockIdx.z * K * C;  // see wgrad_mk_kernel
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < 4; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = k0 + wm * 64 + fm * 16 + 4 * (lane >> 4) + reg;
        int c = c0 + wn * 64 + fn * 16 + (lane & 15);
        if (k < K && c < C) slab[(int64_t)k * C + c] = acc[fm][fn][reg];
      }
}

// --------------------------------------------------------------------------
// Patch wgrad: the im2col matrix is never materialized. The x operand of
// the 128x128 wgrad GEMM is gathered straight from the (channel-padded)
// NHWC input: column index (tap r,s | channel c) decodes to the 16-B
// aligned address ((n*H + oh+r)*W + ow+s)*Cp + c. Removes the global
// im2col pass (2.7 GB write+read at batch 8192 for conv2) entirely;
// concurrent c-tiles of the same m-slice re-read an ~36 KB input window,
// so the repeated taps come from L2, not HBM. Per-tap channel padding to
// Cp = round8(C) keeps every 8-wide load 16-B aligned (the flat layout's
// odd-C columns forced scalar staging).
template <typename T>
DEV_INLINE void wgrad_patch_stage(char* lds, const T* __restrict__ x,
                                  int64_t m0, int64_t M, int H, int W, int OH,
                                  int OW, int S, int Cp, int CRSp, int stride,
                                  int pad, int c0) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int idx = threadIdx.x + i * kBlock;  // 0..2047
    int mi = idx >> 4;                   // m within the 128-round
    int seg = idx & 15;                  // 8-col group
    int col0 = c0 + seg * 8;
    int tap = col0 / Cp;                 // Cp % 8 == 0, col0 % 8 == 0:
    int cin = col0 - tap * Cp;           // a group never crosses a tap
    int r = tap / S, s = tap - (tap / S) * S;
    int64_t m = m0 + mi;
    T vals[8];
    bool ok = (m < M) && (col0 < CRSp);
    int64_t addr = 0;
    if (ok) {
      int64_t n = m / ((int64_t)OH * OW);
      int p = (int)(m - n * OH * OW);
      int oh = p / OW, ow = p - (p / OW) * OW;
      int ih = oh * stride - pad + r, iw = ow * stride - pad + s;
      ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
      addr = ((n * H + ih) * (int64_t)W + iw) * Cp + cin;
    }
    if (ok) {
      *(bf16x8*)vals = *(const bf16x8*)(x + addr);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) vals[j] = from_f32<T>(0.0f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int row = seg * 8 + j;
      *(T*)(lds + row * WG_LSTR + wg_swz(row, mi >> 3) * 16 + (mi & 7) * 2) =
          vals[j];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock)
void conv_wgrad_patch_kernel(const T* __restrict__ gy,
                             const T* __restrict__ x,
                             float* __restrict__ dw /* [z][Kp, CRSp] f32 */,
                             int64_t M, int Kp, int H, int W, int OH, int OW,
                             int S, int Cp, int CRSp, int stride, int pad,
                             int mchunks_per_block) {
  int c0 = blockIdx.x * 128;
  int k0 = blockIdx.y * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* g_lds = smem;                        // [128 k rows][128 m]
  char* x_lds = smem + 128 * WG_LSTR;        // [128 crs rows][128 m]

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);
  f32x4 acc[4][4] = {};

  int64_t m_start = (int64_t)blockIdx.z * mchunks_per_block * WG_BK;
  int64_t m_end = m_start + (int64_t)mchunks_per_block * WG_BK;
  if (m_end > M) m_end = M;

  for (int64_t m0 = m_start; m0 < m_end; m0 += WG_BK) {
    wgrad_mk4_stage(g_lds, gy, m0, M, Kp, k0);
    wgrad_patch_stage(x_lds, x, m0, M, H, W, OH, OW, S, Cp, CRSp, stride,
                      pad, c0);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int fm = 0; fm < 4; ++fm) {
        int arow = wm * 64 + fm * 16 + (lane & 15);
        auto a = *(typename Mma<T>::frag*)(
            g_lds + arow * WG_LSTR +
            wg_swz(arow, ks * 4 + (lane >> 4)) * 16);
#pragma unroll
        for (int fn = 0; fn < 4; ++fn) {
          int brow = wn * 64 + fn * 16 + (lane & 15);
          auto b = *(typename Mma<T>::frag*)(
              x_lds + brow * WG_LSTR +
              wg_swz(brow, ks * 4 + (lane >> 4)) * 16);
          Mma<T>::mma(a, b, acc[fm][fn]);
        }
      }
    }
    __syncthreads();
  }

  float* slab = dw + (int64_t)blockIdx.z * Kp * CRSp;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < 4; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = k0 + wm * 64 + fm * 16 + 4 * (lane >> 4) + reg;
        int c = c0 + wn * 64 + fn * 16 + (lane & 15);
        if (k < Kp && c < CRSp) slab[(int64_t)k * CRSp + c] = acc[fm][fn][reg];
      }
}

// --------------------------------------------------------------------------
// Window-staged patch wgrad (16-bit types). Same GEMM, same partials and the
// same per-element MFMA chain as conv_wgrad_patch_kernel, but both operands
// sit in LDS row-major, as they are in memory, and the fragments (m is the
// contraction index) are formed with the transposed LDS read
// ds_read_b64_tr_b16: two 4-row reads per 8-element fragment.
//   * a block owns one k-tile and up to 384 columns of ONE filter row r
//     (8 waves as 2 k-halves x 4 column groups of 6 fragments). All taps of
//     a filter row read the same input rows, so per 128-m round the x
//     operand is a window of the <= nslots input rows ih = oh*stride-pad+r
//     that the round's output rows touch, staged once at pixel pitch
//     `pitch` with a zero halo of `pad` pixels on both sides. Rows outside
//     the image are staged as zeros and one extra all-zero slot serves
//     m >= M, so padding is an address choice, never a lane mask.
//   * the im2col gather is a per-round table of pixel byte offsets (one
//     entry per m) plus a per-lane constant column offset s*pitch + 2*c;
//     the MFMA loop has no divisions and no selects.
//   * gy is staged [128 m][128 k] with 256-B rows under the XOR swizzle
//     chunk ^= ((row&3)<<2 | (row>>2)&3), which keeps the transposed reads
//     conflict-free; the next round's global loads are issued into
//     registers before the MFMAs of the current one.
// --------------------------------------------------------------------------

constexpr int WW_THREADS = 512;
constexpr int WW_FN = 6;                     // column fragments per wave
constexpr int WW_WCOLS = WW_FN * 16;         // 96 columns per wave
constexpr int WW_COLS = 4 * WW_WCOLS;        // 384 columns per block
constexpr int WW_GY_BYTES = 128 * 256;
constexpr int WW_TAB_BYTES = 128 * 4;
constexpr int WW_XCH = 4;                    // 16-B window chunks per thread
constexpr int WW_MAX_LDS = 144 * 1024;

struct WinGeom {
  int H, W, OH, OW, S, Cp, Kp, CRSp, stride, pad;
  int nslots;       // output rows a 128-m round can touch
  int pitch;        // LDS bytes per pixel (Cp*2, +16 when that is 0 mod 32)
  int slot_bytes;   // (W + 2*pad) * pitch
  int row_chunks;   // W*Cp/8: 16-B chunks of one input row
  int pix_chunks;   // Cp/8
  int ncolblk;      // column blocks per filter row
  int noh;          // N*OH
};

typedef unsigned int ww_u32x4 __attribute__((ext_vector_type(4)));
typedef short ww_s16x4 __attribute__((ext_vector_type(4)));
typedef short ww_s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) ww_s16x4 ww_lds_s16x4;

// 8-element MFMA fragment from two transposed 4-row reads. Every lane of
// the wave must be active and both addresses 8-byte aligned.
template <typename T>
DEV_INLINE typename Mma<T>::frag ww_tr_frag(char* lo_rows, char* hi_rows) {
  ww_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ww_lds_s16x4*)lo_rows);
  ww_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ww_lds_s16x4*)hi_rows);
  ww_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(typename Mma<T>::frag, v);
}

template <typename T>
__global__ __launch_bounds__(WW_THREADS)
void conv_wgrad_window_kernel(const T* __restrict__ gy,
                              const T* __restrict__ x,
                              float* __restrict__ dw /* [z][Kp, CRSp] f32 */,
                              int M, WinGeom g, int mchunks_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* g_lds = smem;                                   // [128 m][128 k]
  int* tab = (int*)(smem + WW_GY_BYTES);                // [128 m] pixel offset
  char* x_lds = smem + WW_GY_BYTES + WW_TAB_BYTES;      // [nslots + 1] rows

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid) / WAVE;  // wave-uniform
  const int wm = wid >> 2, wn = wid & 3;
  const int r = blockIdx.x / g.ncolblk;                 // filter row
  const int cbase = (blockIdx.x - r * g.ncolblk) * WW_COLS;
  const int rowcols = g.S * g.Cp;                       // columns of a filter row
  const int k0 = blockIdx.y * 128;
  const ww_u32x4 zero4 = {0u, 0u, 0u, 0u};

  // halo pixels and the zero slot are written here and never again
  const int xbytes = (g.nslots + 1) * g.slot_bytes;
  for (int o = tid * 16; o < xbytes; o += WW_THREADS * 16)
    *(ww_u32x4*)(x_lds + o) = zero4;

  // this thread's window chunks: the same (slot, pixel, chunk) every round
  const int nchunks = g.nslots * g.row_chunks;
  int xslot[WW_XCH], xdst[WW_XCH], xsrc[WW_XCH];
#pragma unroll
  for (int i = 0; i < WW_XCH; ++i) {
    int idx = tid + i * WW_THREADS;
    int j = idx / g.row_chunks;
    int rc = idx - j * g.row_chunks;
    int px = rc / g.pix_chunks;
    int cc = rc - px * g.pix_chunks;
    xslot[i] = idx < nchunks ? j : -1;
    xdst[i] = j * g.slot_bytes + (g.pad + px) * g.pitch + cc * 16;
    xsrc[i] = rc * 8;
  }

  // transposed-read addresses. Lane 4q+p of a 16-lane group addresses row q,
  // elements 4p..4p+3 of the block; group gq holds m = 32ks + 8gq + 0..7.
  const int gq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int aoff[4][2];
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int row = 8 * gq + 4 * h + q;                     // + 32*ks
      int sw = (q << 2) | ((2 * gq + h) & 3);           // same for every ks
      int ch = wm * 8 + fm * 2 + (p >> 1);
      aoff[fm][h] = 256 * row + 16 * (ch ^ sw) + 8 * (p & 1);
    }
  const int cols_blk = min(WW_COLS, rowcols - cbase);
  int coff[WW_FN];
#pragma unroll
  for (int fn = 0; fn < WW_FN; ++fn) {
    int col = cbase + wn * WW_WCOLS + fn * 16 + 4 * p;
    if (col >= rowcols) col = 0;                        // discarded columns
    int s = col / g.Cp;
    coff[fn] = s * g.pitch + (col - s * g.Cp) * 2;
  }
  const bool wave_on = (k0 + wm * 64 < g.Kp) && (wn * WW_WCOLS < cols_blk);

  f32x4 acc[4][WW_FN] = {};

  const int m_start = blockIdx.z * mchunks_per_block * WG_BK;
  const int m_end = min(m_start + mchunks_per_block * WG_BK, M);

  ww_u32x4 greg[4], xreg[WW_XCH];
  int tabreg = 0;
  auto prefetch = [&](int m0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int idx = tid + i * WW_THREADS;
      int m = m0 + (idx >> 4);
      int k = k0 + (idx & 15) * 8;
      greg[i] = zero4;
      if (m < M && k + 8 <= g.Kp)
        greg[i] = *(const ww_u32x4*)(gy + (int64_t)m * g.Kp + k);
    }
    const int first = m0 / g.OW;                        // first output row
#pragma unroll
    for (int i = 0; i < WW_XCH; ++i) {
      int orow = first + xslot[i];
      int n = orow / g.OH;
      int ih = (orow - n * g.OH) * g.stride - g.pad + r;
      bool ok = xslot[i] >= 0 && orow < g.noh && ih >= 0 && ih < g.H;
      xreg[i] = zero4;
      if (ok)
        xreg[i] = *(const ww_u32x4*)(x + ((int64_t)(n * g.H + ih) * g.W) * g.Cp +
                                     xsrc[i]);
    }
    if (tid < 128) {
      int m = m0 + tid;
      int orow = m / g.OW;
      tabreg = m < M ? (orow - first) * g.slot_bytes +
                           (m - orow * g.OW) * g.stride * g.pitch
                     : g.nslots * g.slot_bytes;         // the zero slot
    }
  };

  if (m_start < m_end) prefetch(m_start);
  __syncthreads();                                      // window zeroed

  for (int m0 = m_start; m0 < m_end; m0 += WG_BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int idx = tid + i * WW_THREADS;
      int mi = idx >> 4, ch = idx & 15;
      *(ww_u32x4*)(g_lds + 256 * mi +
                16 * (ch ^ (((mi & 3) << 2) | ((mi >> 2) & 3)))) = greg[i];
    }
#pragma unroll
    for (int i = 0; i < WW_XCH; ++i)
      if (xslot[i] >= 0) *(ww_u32x4*)(x_lds + xdst[i]) = xreg[i];
    if (tid < 128) tab[tid] = tabreg;
    __syncthreads();
    if (m0 + WG_BK < m_end) prefetch(m0 + WG_BK);
    if (wave_on) {
      int po[4][2];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int h = 0; h < 2; ++h) po[ks][h] = tab[32 * ks + 8 * gq + 4 * h + q];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        typename Mma<T>::frag a[4];
#pragma unroll
        for (int fm = 0; fm < 4; ++fm)
          a[fm] = ww_tr_frag<T>(g_lds + aoff[fm][0] + ks * 8192,
                                g_lds + aoff[fm][1] + ks * 8192);
#pragma unroll
        for (int fn = 0; fn < WW_FN; ++fn) {
          auto b = ww_tr_frag<T>(x_lds + po[ks][0] + coff[fn],
                                 x_lds + po[ks][1] + coff[fn]);
#pragma unroll
          for (int fm = 0; fm < 4; ++fm) Mma<T>::mma(a[fm], b, acc[fm][fn]);
        }
      }
    }
    __syncthreads();
  }

  if (!wave_on) return;
  float* slab = dw + (int64_t)blockIdx.z * g.Kp * g.CRSp +
                (int64_t)r * rowcols;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < WW_FN; ++fn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int k = k0 + wm * 64 + fm * 16 + 4 * gq + reg;
        int c = cbase + wn * WW_WCOLS + fn * 16 + (lane & 15);
        if (k < g.Kp && c < rowcols)
          slab[(int64_t)k * g.CRSp + c] = acc[fm][fn][reg];
      }
}

// Shapes the window kernel takes: the window of one round (plus the zero
// slot) and the gy tile fit the LDS budget, and no thread stages more than
// WW_XCH chunks of it. N only enters through `noh` and the int32 m.
bool ww_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t K, int64_t R,
             int64_t S, int64_t stride, int64_t pad, int64_t elem_size,
             WinGeom* out) {
  if (elem_size != 2 || stride < 1 || pad < 0) return false;
  if (H + 2 * pad < R || W + 2 * pad < S) return false;
  int64_t OH = (H + 2 * pad - R) / stride + 1;
  int64_t OW = (W + 2 * pad - S) / stride + 1;
  int64_t Cp = (C + 7) & ~(int64_t)7, Kp = (K + 7) & ~(int64_t)7;
  int64_t nslots = (OW + 126) / OW + 1;
  int64_t pitch = Cp * 2 + ((Cp * 2) % 32 == 0 ? 16 : 0);
  int64_t slot_bytes = (W + 2 * pad) * pitch;
  int64_t row_chunks = W * Cp / 8;
  if (nslots * row_chunks > (int64_t)WW_XCH * WW_THREADS) return false;
  if (WW_GY_BYTES + WW_TAB_BYTES + (nslots + 1) * slot_bytes > WW_MAX_LDS)
    return false;
  if (N * OH * OW > (int64_t)INT32_MAX - 2 * WG_BK ||
      R * S * Cp * Kp > (int64_t)INT32_MAX)
    return false;
  if (out) {
    WinGeom g;
    g.H = (int)H; g.W = (int)W; g.OH = (int)OH; g.OW = (int)OW; g.S = (int)S;
    g.Cp = (int)Cp; g.Kp = (int)Kp; g.CRSp = (int)(R * S * Cp);
    g.stride = (int)stride; g.pad = (int)pad; g.nslots = (int)nslots;
    g.pitch = (int)pitch; g.slot_bytes = (int)slot_bytes;
    g.row_chunks = (int)row_chunks; g.pix_chunks = (int)(Cp / 8);
    g.ncolblk = (int)((S * Cp + WW_COLS - 1) / WW_COLS);
    g.noh = (int)(N * OH);
    *out = g;
  }
  return true;
}

bool ww_forced_legacy() {
  const char* e = getenv("NOISYNET_WGRAD_PATCH");
  return e != nullptr && std::string(e) == "legacy";
}

}  // namespace

// ===========================================================================
// host wrappers
// ===========================================================================

torch::Tensor conv_fwd(torch::Tensor x, torch::Tensor w, int64_t stride,
                       int64_t pad) {
  check_cl(x, "conv_fwd x");
  check_cl(w, "conv_fwd w");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)w.size(0), (int)w.size(2),
                     (int)w.size(3), (int)stride, (int)pad);
  auto out = torch::empty({g.N, g.K, g.OH, g.OW},
                          x.options().memory_format(at::MemoryFormat::ChannelsLast));
  dim3 grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(x.scalar_type(),
                                  "conv_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + BN) * Mma<T>::STRIDE;
    hipLaunchKernelGGL((conv_fwd_kernel<T, true, 0, false, false>), grid,
                       dim3(kBlock), lds, c10::hip::getCurrentHIPStream(),
                       (const T*)x.data_ptr(), (const T*)w.data_ptr(),
                       (const T*)w.data_ptr(), nullptr, (T*)out.data_ptr(), g,
                       nullptr, 0, nullptr);
  });
  HIP_CHECK_LAST();
  return out;
}

std::vector<torch::Tensor> conv_fwd_fused_impl(torch::Tensor x,
                                               torch::Tensor wq,
                                               torch::Tensor wraw,
                                               torch::Tensor bias,
                                               int64_t stride, int64_t pad,
                                               int64_t sigma_mode,
                                               torch::Tensor factor,
                                               int64_t seed,
                                               bool telem, bool want_y) {
  check_sigma_mode(sigma_mode, false, "conv_fwd_fused (streaming route)");
  check_cl(x, "conv_fwd_fused x");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)wraw.size(0), (int)wraw.size(2),
                     (int)wraw.size(3), (int)stride, (int)pad);
  auto out = torch::empty({g.N, g.K, g.OH, g.OW},
                          x.options().memory_format(at::MemoryFormat::ChannelsLast));
  bool has_bias = bias.numel() > 0;
  torch::Tensor bias_f;
  if (has_bias) bias_f = bias.to(torch::kFloat32).contiguous();
  // telemetry buffer only when requested (steady-state training has
  // telem=false; the zeros+fill launches were ~12 tiny kernels/step)
  auto tele = telem
      ? [&] {
          auto t = torch::zeros({3}, x.options().dtype(torch::kFloat32));
          t[2] = -std::numeric_limits<float>::infinity();
          return t;
        }()
      : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();
  dim3 grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(x.scalar_type(),
                                  "conv_fwd_fused", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + 3 * BN) * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq.data_ptr();
    const T* wrp = (const T*)wraw.data_ptr();
    const float* bp = has_bias ? bias_f.data_ptr<float>() : nullptr;
    T* op = (T*)out.data_ptr();
    float* tp = telem ? tele.data_ptr<float>() : nullptr;
    const float* f = factor_f.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    auto launch = [&](auto wy, auto sm, auto tl, auto bi) {
      hipLaunchKernelGGL((conv_fwd_kernel<T, decltype(wy)::value,
                          decltype(sm)::value, decltype(tl)::value,
                          decltype(bi)::value>), grid, dim3(kBlock), lds,
                         stream, xp, wqp, wrp, bp, op, g, f, sd, tp, g_seed_base);
    };
    using TT = std::true_type; using FF = std::false_type;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    if (want_y) {
      if (sigma_mode == 1) {
        if (telem) { if (has_bias) launch(TT{}, S1{}, TT{}, TT{}); else launch(TT{}, S1{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S1{}, FF{}, TT{}); else launch(TT{}, S1{}, FF{}, FF{}); }
      } else {
        if (telem) { if (has_bias) launch(TT{}, S2{}, TT{}, TT{}); else launch(TT{}, S2{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S2{}, FF{}, TT{}); else launch(TT{}, S2{}, FF{}, FF{}); }
      }
    } else {
      if (sigma_mode == 1) {
        if (telem) launch(FF{}, S1{}, TT{}, FF{}); else launch(FF{}, S1{}, FF{}, FF{});
      } else {
        if (telem) launch(FF{}, S2{}, TT{}, FF{}); else launch(FF{}, S2{}, FF{}, FF{});
      }
    }
  });
  HIP_CHECK_LAST();
  return {out, tele};
}

torch::Tensor conv_dgrad(torch::Tensor gy, torch::Tensor w, int64_t stride,
                         int64_t pad, int64_t H, int64_t W) {
  check_cl(gy, "conv_dgrad gy");
  check_cl(w, "conv_dgrad w");
  auto g = make_geom((int)gy.size(0), (int)H, (int)W, (int)w.size(1),
                     (int)w.size(0), (int)w.size(2), (int)w.size(3),
                     (int)stride, (int)pad);
  TORCH_CHECK(g.OH == (int)gy.size(2) && g.OW == (int)gy.size(3),
              "conv_dgrad: grad shape mismatch");
  // wt[r,s,c,k]: contraction-contiguous weight view (tiny tensor)
  auto wt = w.permute({2, 3, 1, 0}).contiguous();
  auto dx = torch::empty({g.N, g.C, g.H, g.W},
                         gy.options().memory_format(at::MemoryFormat::ChannelsLast));
  int64_t MI = (int64_t)g.N * g.H * g.W;
  dim3 grid((g.C + BN - 1) / BN, (int)((MI + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(gy.scalar_type(),
                                  "conv_dgrad", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + BN) * Mma<T>::STRIDE;
    hipLaunchKernelGGL((conv_dgrad_kernel<T>), grid, dim3(kBlock), lds,
                       c10::hip::getCurrentHIPStream(),
                       (const T*)gy.data_ptr(), (const T*)wt.data_ptr(),
                       (T*)dx.data_ptr(), g);
  });
  HIP_CHECK_LAST();
  return dx;
}

torch::Tensor conv_wgrad(torch::Tensor gy, torch::Tensor x, int64_t stride,
                         int64_t pad, int64_t R, int64_t S) {
  check_cl(gy, "conv_wgrad gy");
  check_cl(x, "conv_wgrad x");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)gy.size(1), (int)R, (int)S,
                     (int)stride, (int)pad);
  // slice the contraction so ~2048 blocks are in flight
  int taps = g.flat ? 1 : g.R * g.S;
  int span = g.flat ? g.R * g.S * g.C : g.C;
  int64_t mtotal = (g.M + BK - 1) / BK;  // number of BK chunks
  int ctiles = (span + BN - 1) / BN;
  int ktiles = (g.K + BM - 1) / BM;
  int64_t target_z = std::max<int64_t>(1, 2048 / std::max(1, ctiles * ktiles));
  int mslices = (int)std::min<int64_t>(
      mtotal, std::max<int64_t>(1, target_z / taps));
  int chunks_per_block = (int)((mtotal + mslices - 1) / mslices);
  // per-mslice partial weight images, summed by torch in fixed order
  // (deterministic; the atomicAdd variant gave run-to-run noise)
  auto dw_f = torch::zeros({mslices, g.K, g.R, g.S, g.C},
                           x.options().dtype(torch::kFloat32));
  int64_t wspan = (int64_t)g.K * g.R * g.S * g.C;
  dim3 grid(ctiles, ktiles, taps * mslices);
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(gy.scalar_type(),
                                  "conv_wgrad", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + BN) * Mma<T>::STRIDE;
    hipLaunchKernelGGL((conv_wgrad_kernel<T>), grid, dim3(kBlock), lds,
                       c10::hip::getCurrentHIPStream(),
                       (const T*)gy.data_ptr(), (const T*)x.data_ptr(),
                       dw_f.data_ptr<float>(), g, chunks_per_block, wspan);
  });
  HIP_CHECK_LAST();
  // dw as NCHW-logical [K, C, R, S] channels_last == raw [K,R,S,C]
  auto dw = dw_f.sum(0).to(x.scalar_type());
  return dw.permute({0, 3, 1, 2}).contiguous(at::MemoryFormat::ChannelsLast);
}

// ===========================================================================
// Linear layers = the R=S=1, H=W=1 case: a 2-D row-major [B, F] tensor has
// exactly the raw layout of an NHWC (B, F, 1, 1) channels_last tensor, so
// the conv kernels run unchanged on raw pointers.
// ===========================================================================

torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w) {
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  auto g = linear_geom(x, w.size(0));
  auto out = torch::empty({x.size(0), w.size(0)}, x.options());
  dim3 grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(x.scalar_type(),
                                  "linear_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + BN) * Mma<T>::STRIDE;
    hipLaunchKernelGGL((conv_fwd_kernel<T, true, 0, false, false>), grid,
                       dim3(kBlock), lds, c10::hip::getCurrentHIPStream(),
                       (const T*)x.data_ptr(), (const T*)w.data_ptr(),
                       (const T*)w.data_ptr(), nullptr, (T*)out.data_ptr(), g,
                       nullptr, 0, nullptr);
  });
  HIP_CHECK_LAST();
  return out;
}

// dx = g @ W: contraction over out_features -> conv_fwd with A=g [B,O] and
// "weights" = W^T [I, O] (pre-transposed; W is small).
torch::Tensor linear_dgrad(torch::Tensor gy, torch::Tensor w) {
  auto wt = w.t().contiguous();  // [I, O]
  return linear_fwd(gy, wt);
}

// dW = g^T @ x: the wgrad kernel with the 1x1-tap geometry.
torch::Tensor linear_wgrad(torch::Tensor gy, torch::Tensor x) {
  TORCH_CHECK(gy.dim() == 2 && gy.is_contiguous());
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous());
  auto g = linear_geom(x, gy.size(1));
  if ((g.K & 7) == 0 && (g.C & 7) == 0 && gy.element_size() == 2) {
    // aligned 16-bit: 128-deep rounds. Wide outputs use the 128x128-tile
    // variant (fewer cross-tile operand re-reads); narrow ones the
    // 64x64 with a register pipeline.
    bool wide = (int64_t)g.C * g.K >= 128 * 1024;
    int tn = wide ? 128 : BN;
    int tm = wide ? 128 : BM;
    int ctiles = (g.C + tn - 1) / tn;
    int ktiles = (g.K + tm - 1) / tm;
    int64_t mtotal = (g.M + WG_BK - 1) / WG_BK;
    int64_t target_z =
        std::max<int64_t>(1, 2048 / std::max(1, ctiles * ktiles));
    int chunks = (int)((mtotal + target_z - 1) / target_z);
    int mslices = (int)((mtotal + chunks - 1) / chunks);  // no empty slices
    dim3 grid(ctiles, ktiles, mslices);
    size_t lds = (size_t)(tm + tn) * WG_LSTR;
    // per-slice partials, plain stores, deterministic sum
    auto parts = torch::empty({(int64_t)mslices, (int64_t)g.K * g.C},
                              x.options().dtype(torch::kFloat32));
    NN_DISPATCH(gy.scalar_type(), "linear_wgrad_mk", [&] {
      using T = typename DevT<scalar_t>::type;
      if (wide) {
        hipLaunchKernelGGL((wgrad_mk4_kernel<T>), grid, dim3(kBlock), lds,
                           c10::hip::getCurrentHIPStream(),
                           (const T*)gy.data_ptr(), (const T*)x.data_ptr(),
                           parts.data_ptr<float>(), g.M, g.K, g.C, chunks);
      } else {
        hipLaunchKernelGGL((wgrad_mk_kernel<T>), grid, dim3(kBlock), lds,
                           c10::hip::getCurrentHIPStream(),
                           (const T*)gy.data_ptr(), (const T*)x.data_ptr(),
                           parts.data_ptr<float>(), g.M, g.K, g.C, chunks);
      }
    });
    HIP_CHECK_LAST();
    return parts.sum(0).view({(int64_t)g.K, (int64_t)g.C})
        .to(x.scalar_type());
  }
  int64_t mtotal = (g.M + BK - 1) / BK;
  int ctiles = (g.C + BN - 1) / BN;
  int ktiles = (g.K + BM - 1) / BM;
  int64_t target_z = std::max<int64_t>(1, 1024 / std::max(1, ctiles * ktiles));
  int mslices = (int)std::min<int64_t>(mtotal, target_z);
  if (mslices < 1) mslices = 1;
  int chunks_per_block = (int)((mtotal + mslices - 1) / mslices);
  dim3 grid(ctiles, ktiles, mslices);
  // per-mslice partials, deterministic fixed-order sum (see conv_wgrad)
  auto parts_f = torch::zeros({mslices, g.K, g.C},
                              x.options().dtype(torch::kFloat32));
  int64_t wspan = (int64_t)g.K * g.C;
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(gy.scalar_type(),
                                  "linear_wgrad", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + BN) * Mma<T>::STRIDE;
    hipLaunchKernelGGL((conv_wgrad_kernel<T>), grid, dim3(kBlock), lds,
                       c10::hip::getCurrentHIPStream(),
                       (const T*)gy.data_ptr(), (const T*)x.data_ptr(),
                       parts_f.data_ptr<float>(), g, chunks_per_block, wspan);
  });
  HIP_CHECK_LAST();
  return parts_f.sum(0).to(x.scalar_type());
}

namespace {

// Route of the fused noisy GEMM out[M,K] = x[M,Kc] @ w[K,Kc]^T. The one
// place the choice is made: linear_fwd_fused / sigma_noise_linear dispatch
// on it and linear_fused_route reports it.
enum class LinearRoute { SmallK, Gemm };

LinearRoute linear_route(int64_t Kc, int64_t K, int64_t elem_size) {
  // small-K kernel (see conv_fwd_smallk_kernel); Kc % 32 == 0: its A/W
  // staging loads carry no column bounds checks
  if (Kc <= 128 && (Kc & 31) == 0 && K <= 96 && elem_size == 2)
    return LinearRoute::SmallK;
  return LinearRoute::Gemm;
}

bool smallk_eligible(const torch::Tensor& x, int64_t K) {
  return linear_route(x.size(1), K, (int64_t)x.element_size()) ==
         LinearRoute::SmallK;
}

}  // namespace

// The fused kernels are instantiated for sigma_mode 1 (|w|) and 2
// (|w|^2+|w|); a noise-free mode 0 exists only where allow_zero says so.
// Anything else used to fall through to the mode-2 launch. (Declared in
// mfma_tile.h: the crossbar translation units call it too.)
void check_sigma_mode(int64_t sigma_mode, bool allow_zero, const char* who) {
  TORCH_CHECK(sigma_mode == 1 || sigma_mode == 2 ||
                  (allow_zero && sigma_mode == 0),
              who, ": sigma_mode ", sigma_mode, " is not supported here (",
              allow_zero ? "0, " : "", "1 or 2)");
}

namespace {

std::vector<torch::Tensor> linear_fwd_fused_smallk(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t sigma_mode, torch::Tensor factor, int64_t seed, bool telem,
    bool want_y) {
  // the noise-free S0 variant exists with the y accumulator only
  check_sigma_mode(sigma_mode, want_y, "linear_fwd_fused_smallk");
  int64_t M = x.size(0);
  int K = (int)wraw.size(0);
  int Kc = (int)x.size(1);
  int CH = (Kc + 31) >> 5;
  // the kernel stages a fixed 96-row weight image with no row bounds
  // checks: pad the (tiny) weight tensors with zero rows
  if (K < 96) {
    wraw = at::constant_pad_nd(wraw, {0, 0, 0, 96 - K}, 0);
    if (want_y) wq = at::constant_pad_nd(wq, {0, 0, 0, 96 - K}, 0);
    else wq = wraw;
  }
  auto out = torch::empty({M, (int64_t)K}, x.options());
  bool has_bias = bias.numel() > 0;
  torch::Tensor bias_f;
  if (has_bias) bias_f = bias.to(torch::kFloat32).contiguous();
  auto tele = telem
      ? [&] {
          auto t = torch::zeros({3}, x.options().dtype(torch::kFloat32));
          t[2] = -std::numeric_limits<float>::infinity();
          return t;
        }()
      : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();
  int64_t mtiles = (M + BM - 1) / BM;
  int blocks = (int)std::min<int64_t>(mtiles, 8192);
  NN_DISPATCH(x.scalar_type(), "linear_fwd_fused_smallk", [&] {
    using T = typename DevT<scalar_t>::type;
    bool d_live = telem && sigma_mode == 2;
    size_t lds = (size_t)CH * Mma<T>::STRIDE * (BM + 96 * (d_live ? 3 : 2));
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq.data_ptr();
    const T* wrp = (const T*)wraw.data_ptr();
    const float* bp = has_bias ? bias_f.data_ptr<float>() : nullptr;
    T* op = (T*)out.data_ptr();
    float* tp = telem ? tele.data_ptr<float>() : nullptr;
    const float* f = factor_f.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    auto launch = [&](auto wy, auto sm, auto tl, auto bi) {
      auto* kfn = &conv_fwd_smallk_kernel<T, decltype(wy)::value,
                                          decltype(sm)::value,
                                          decltype(tl)::value,
                                          decltype(bi)::value>;
      if (lds > 64 * 1024)
        hipFuncSetAttribute((const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
      hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kBlock), lds, stream, xp,
                         wqp, wrp, bp, op, M, K, Kc, f, sd, tp, g_seed_base);
    };
    using TT = std::true_type; using FF = std::false_type;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    if (want_y) {
      if (sigma_mode == 0) {
        if (has_bias) launch(TT{}, S0{}, FF{}, TT{});
        else launch(TT{}, S0{}, FF{}, FF{});
      } else if (sigma_mode == 1) {
        if (telem) { if (has_bias) launch(TT{}, S1{}, TT{}, TT{}); else launch(TT{}, S1{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S1{}, FF{}, TT{}); else launch(TT{}, S1{}, FF{}, FF{}); }
      } else {
        if (telem) { if (has_bias) launch(TT{}, S2{}, TT{}, TT{}); else launch(TT{}, S2{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S2{}, FF{}, TT{}); else launch(TT{}, S2{}, FF{}, FF{}); }
      }
    } else {
      if (sigma_mode == 1) {
        if (telem) launch(FF{}, S1{}, TT{}, FF{}); else launch(FF{}, S1{}, FF{}, FF{});
      } else {
        if (telem) launch(FF{}, S2{}, TT{}, FF{}); else launch(FF{}, S2{}, FF{}, FF{});
      }
    }
  });
  HIP_CHECK_LAST();
  return {out, tele};
}

}  // namespace

std::vector<torch::Tensor> linear_fwd_fused(torch::Tensor x, torch::Tensor wq,
                                            torch::Tensor wraw,
                                            torch::Tensor bias,
                                            int64_t sigma_mode,
                                            torch::Tensor factor,
                                            int64_t seed, bool telem) {
  if (smallk_eligible(x, wraw.size(0)))
    return linear_fwd_fused_smallk(x, wq, wraw, bias, sigma_mode, factor,
                                   seed, telem, /*want_y=*/true);
  check_sigma_mode(sigma_mode, false, "linear_fwd_fused");
  auto g = linear_geom(x, wraw.size(0));
  // row-pad the (small) weight matrices to the 64-row k-tile multiple so
  // the staging guard k < Kw never diverges inside a tile (the masked
  // scalar fallback serializes a vmcnt(0) per element)
  int k_pad = (g.K + BM - 1) / BM * BM;
  if (k_pad != g.K && wraw.element_size() == 2) {
    wq = at::constant_pad_nd(wq, {0, 0, 0, k_pad - g.K}, 0);
    wraw = at::constant_pad_nd(wraw, {0, 0, 0, k_pad - g.K}, 0);
    g.Kw = k_pad;
  }
  // NOTE: out/geometry use g.K (the logical row count), never the
  // possibly row-padded wraw.size(0)
  auto out = torch::empty({x.size(0), (int64_t)g.K}, x.options());
  bool has_bias = bias.numel() > 0;
  torch::Tensor bias_f;
  if (has_bias) bias_f = bias.to(torch::kFloat32).contiguous();
  // telemetry buffer only when requested (steady-state training has
  // telem=false; the zeros+fill launches were ~12 tiny kernels/step)
  auto tele = telem
      ? [&] {
          auto t = torch::zeros({3}, x.options().dtype(torch::kFloat32));
          t[2] = -std::numeric_limits<float>::infinity();
          return t;
        }()
      : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();
  dim3 grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(x.scalar_type(),
                                  "linear_fwd_fused", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + 3 * BN) * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq.data_ptr();
    const T* wrp = (const T*)wraw.data_ptr();
    const float* bp = has_bias ? bias_f.data_ptr<float>() : nullptr;
    T* op = (T*)out.data_ptr();
    float* tp = telem ? tele.data_ptr<float>() : nullptr;
    const float* f = factor_f.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    auto launch = [&](auto sm, auto tl, auto bi) {
      hipLaunchKernelGGL((conv_fwd_kernel<T, true, decltype(sm)::value,
                          decltype(tl)::value, decltype(bi)::value>), grid,
                         dim3(kBlock), lds, stream, xp, wqp, wrp, bp, op, g,
                         f, sd, tp, g_seed_base);
    };
    using TT = std::true_type; using FF = std::false_type;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    if (sigma_mode == 1) {
      if (telem) { if (has_bias) launch(S1{}, TT{}, TT{}); else launch(S1{}, TT{}, FF{}); }
      else { if (has_bias) launch(S1{}, FF{}, TT{}); else launch(S1{}, FF{}, FF{}); }
    } else {
      if (telem) { if (has_bias) launch(S2{}, TT{}, TT{}); else launch(S2{}, TT{}, FF{}); }
      else { if (has_bias) launch(S2{}, FF{}, TT{}); else launch(S2{}, FF{}, FF{}); }
    }
  });
  HIP_CHECK_LAST();
  return {out, tele};
}

std::vector<torch::Tensor> sigma_noise_linear_impl(torch::Tensor x,
                                                   torch::Tensor wraw,
                                                   int64_t sigma_mode,
                                                   torch::Tensor factor,
                                                   int64_t seed,
                                                   bool telem) {
  if (smallk_eligible(x, wraw.size(0))) {
    auto empty_bias = torch::empty({0}, x.options());
    return linear_fwd_fused_smallk(x, wraw, wraw, empty_bias, sigma_mode,
                                   factor, seed, telem, /*want_y=*/false);
  }
  check_sigma_mode(sigma_mode, false, "sigma_noise_linear");
  auto g = linear_geom(x, wraw.size(0));
  auto out = torch::empty({x.size(0), (int64_t)g.K}, x.options());
  // telemetry buffer only when requested (steady-state training has
  // telem=false; the zeros+fill launches were ~12 tiny kernels/step)
  auto tele = telem
      ? [&] {
          auto t = torch::zeros({3}, x.options().dtype(torch::kFloat32));
          t[2] = -std::numeric_limits<float>::infinity();
          return t;
        }()
      : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();
  dim3 grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM));
  size_t lds = 0;  // per-dtype, set inside the dispatch
  NN_DISPATCH(x.scalar_type(),
                                  "sigma_noise_linear", [&] {
    using T = typename DevT<scalar_t>::type;
    lds = (size_t)(BM + 3 * BN) * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wrp = (const T*)wraw.data_ptr();
    T* op = (T*)out.data_ptr();
    float* tp = telem ? tele.data_ptr<float>() : nullptr;
    const float* f = factor_f.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    if (sigma_mode == 1) {
      if (telem)
        hipLaunchKernelGGL((conv_fwd_kernel<T, false, 1, true, false>), grid,
                           dim3(kBlock), lds, stream, xp, wrp, wrp, nullptr,
                           op, g, f, sd, tp, g_seed_base);
      else
        hipLaunchKernelGGL((conv_fwd_kernel<T, false, 1, false, false>), grid,
                           dim3(kBlock), lds, stream, xp, wrp, wrp, nullptr,
                           op, g, f, sd, tp, g_seed_base);
    } else {
      if (telem)
        hipLaunchKernelGGL((conv_fwd_kernel<T, false, 2, true, false>), grid,
                           dim3(kBlock), lds, stream, xp, wrp, wrp, nullptr,
                           op, g, f, sd, tp, g_seed_base);
      else
        hipLaunchKernelGGL((conv_fwd_kernel<T, false, 2, false, false>), grid,
                           dim3(kBlock), lds, stream, xp, wrp, wrp, nullptr,
                           op, g, f, sd, tp, g_seed_base);
    }
  });
  HIP_CHECK_LAST();
  return {out, tele};
}

std::string linear_fused_route(int64_t Kc, int64_t K, int64_t elem_size) {
  return linear_route(Kc, K, elem_size) == LinearRoute::SmallK ? "smallk"
                                                               : "gemm";
}

// ===========================================================================
// Image-patch conv forward: the whole (zero-padded) input image lives in LDS
// for the block's lifetime, so the K-loop re-reads it from LDS instead of
// re-gathering from HBM once per tap (the streaming kernel above reads each
// input pixel R*S times). Contraction runs per filter ROW over the
// (s, c)-contiguous span S*C_pad, which is contiguous BOTH in the padded
// patch and in the channel-padded weights -> every fragment is an aligned
// ds_read_b128 / 16-B weight load.
//
// Eligible when H_pad*W_pad*C_pad*2 fits the LDS budget -- exactly the
// CIFAR-scale layers (conv2: 14x14x65 -> 28 KB patch) whose C=65 defeats
// vectorized NHWC staging in the streaming kernel.
// ===========================================================================

namespace {

struct PatchGeom {
  int C_pad;   // channels padded to a multiple of 8
  int Wp;      // W + 2*pad (patch holds the horizontal borders)
  int Kr;      // per-row contraction length = S * C_pad
  int Krs;     // padded weight row stride = round32(Kr) (zero tail)
  int MI;      // outputs per image = OH * OW
};

template <typename T>
DEV_INLINE void stage_patch(char* patch, const T* __restrict__ x,
                            const ConvGeom g, const PatchGeom p, int n) {
  constexpr int EB = (int)sizeof(T) == 4 ? 4 : 2;
  int total = g.H * p.Wp * p.C_pad;
  const T* img = x + (int64_t)n * g.H * g.W * g.C;
  bool vec = (sizeof(T) == 2) && ((g.C & 7) == 0);
  if (vec) {
    // 8-element vector spans within a pixel
    int spans = total / 8;
    for (int sidx = threadIdx.x; sidx < spans; sidx += blockDim.x) {
      int idx = sidx * 8;
      int c = idx % p.C_pad;
      int pix = idx / p.C_pad;
      int iwp = pix % p.Wp;
      int ih = pix / p.Wp;
      int iw = iwp - g.pad;
      bf16x8 v;
      if (iw >= 0 && iw < g.W && c + 8 <= g.C) {
        v = *(const bf16x8*)(img + ((int64_t)ih * g.W + iw) * g.C + c);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) ((bf16*)&v)[j] = __float2bfloat16(0.0f);
      }
      *(bf16x8*)(patch + (int64_t)idx * 2) = v;
    }
  } else {
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      int c = idx % p.C_pad;
      int pix = idx / p.C_pad;
      int iwp = pix % p.Wp;
      int ih = pix / p.Wp;
      int iw = iwp - g.pad;
      float v = 0.0f;
      if (iw >= 0 && iw < g.W && c < g.C)
        v = to_f32(img[((int64_t)ih * g.W + iw) * g.C + c]);
      ((T*)patch)[idx] = from_f32<T>(v);
    }
  }
  // zero slot at patch end for out-of-bounds fragment reads (one full
  // 32-element span of the compute type)
  if (threadIdx.x < 8) {
    char* z = patch + (int64_t)g.H * p.Wp * p.C_pad * EB + threadIdx.x * 16;
    *(bf16x8*)z = bf16x8{};
  }
}

// register-pipelined weight staging: load the next chunk's values into
// registers during the MFMA phase (the synchronous stage->barrier->mma
// structure exposed the full global-load latency every round; PMC showed
// 65% of wave-cycles parked). One wraw load feeds both the sigma and the
// telemetry |w| stores.
//
// The weight image is FULLY padded host-side (rows to the k-tile
// multiple, columns to round32(Kr), all zeros) so this load is one
// UNCONDITIONAL 16-B vector: the earlier bounds-checked fallback
// compiled to 16 exec-masked global_load_ushort each trailed by
// s_waitcnt vmcnt(0) -- a serial latency storm on every round for any
// block touching a tile edge.
template <typename T>
DEV_INLINE void load_wrow_regs(T dst[8], const T* __restrict__ w,
                               const ConvGeom g, const PatchGeom p, int n0,
                               int r, int ck) {
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  int k = n0 + row;
  const T* src = w + ((int64_t)k * g.R + r) * p.Krs + ck + seg * 8;
  if (sizeof(T) == 2) {
    *(bf16x8*)dst = *(const bf16x8*)src;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = src[j];
  }
}

template <typename T, bool ABS_TRANSFORM, int SIGMA_MODE>
DEV_INLINE void store_wrow_regs(char* lds, const T src[8]) {
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  if (!ABS_TRANSFORM && sizeof(T) == 2) {
    *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) = *(const bf16x8*)src;
    return;
  }
  float vals[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = to_f32(src[j]);
    if (ABS_TRANSFORM) {
      v = fabsf(v);
      if (SIGMA_MODE == 2) v = v * v + v;
    }
    vals[j] = v;
  }
  Mma<T>::store8(lds, row, seg * 8, vals);
}

template <typename T, bool WANT_Y, int SIGMA_MODE, bool TELEM, bool BIAS>
__global__ __launch_bounds__(kBlock)
void conv_fwd_patch_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                           const T* __restrict__ wraw,
                           const float* __restrict__ bias,
                           T* __restrict__ out, ConvGeom g, PatchGeom p,
                           const float* __restrict__ factor_p, uint64_t seed,
                           float* __restrict__ telem,
                           const int64_t* __restrict__ seed_base = nullptr) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  constexpr int EB = (int)sizeof(T) == 4 ? 4 : 2;
  constexpr int STR = Mma<T>::STRIDE;
  int n0 = blockIdx.x * BN;   // output-channel tile
  int n = blockIdx.y;         // image

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* patch = smem;  // H * Wp * C_pad elements + one zero span
  size_t patch_bytes = (size_t)g.H * p.Wp * p.C_pad * EB + 128;
  char* b_lds = smem + patch_bytes;
  char* c_lds = b_lds + BN * STR;
  char* d_lds = c_lds + BN * STR;
  int64_t zero_off = (int64_t)g.H * p.Wp * p.C_pad * EB;

  stage_patch(patch, x, g, p, n);

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  float t_sum_sigma = 0.0f, t_sum_noise = 0.0f, t_max_y = -INFINITY;

  const int CHW = (p.Kr + BK - 1) / BK;
  const int ROUNDS = g.R * CHW;
  T breg[8], creg[8];
  if (WANT_Y) load_wrow_regs(breg, wq, g, p, n0, 0, 0);
  if (SIGMA_MODE > 0) load_wrow_regs(creg, wraw, g, p, n0, 0, 0);

  // M-subtiles share each staged weight tile (fewer barriers). A plain
  // conv (dgrad-via-patch) carries only the y accumulators, so it can
  // afford 4 subtiles (196-pixel images finish in ONE weight pass);
  // sigma variants carry 2-3 accumulator sets and stay at 2.
  constexpr int MSUB = (SIGMA_MODE == 0) ? 4 : 2;
  for (int m0 = 0; m0 < p.MI; m0 += MSUB * BM) {
    f32x4 acc[MSUB][2][2] = {};
    f32x4 sacc[MSUB][2][2] = {};
    f32x4 tacc[MSUB][2][2] = {};
    int rem = (int)((p.MI - m0 + BM - 1) / BM);
    const int nsub = rem < MSUB ? rem : MSUB;

    // hoist the per-fragment pixel decode: ow/oh (integer divisions) and
    // the patch base offset are invariant across the (r, ck) rounds
    int a_ohs[MSUB][2];   // oh*stride - pad, or INT_MIN when m >= MI
    int a_base[MSUB][2];  // ((ohs*Wp + ow*stride) * C_pad) element offset
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
        int m_local = m0 + ms * BM + wm * 32 + fm * 16 + (lane & 15);
        if (m_local < p.MI) {
          int ow = m_local % g.OW;
          int oh = m_local / g.OW;
          int ohs = oh * g.stride - g.pad;
          a_ohs[ms][fm] = ohs;
          a_base[ms][fm] = (ohs * p.Wp + ow * g.stride) * p.C_pad;
        } else {
          a_ohs[ms][fm] = INT_MIN / 2;
          a_base[ms][fm] = 0;
        }
      }
    const int rowpitch = p.Wp * p.C_pad;

    int r = 0, ck = 0;
    for (int t = 0; t < ROUNDS; ++t) {
      {
        if (WANT_Y) store_wrow_regs<T, false, 0>(b_lds, breg);
        if (SIGMA_MODE > 0)
          store_wrow_regs<T, true, SIGMA_MODE>(c_lds, creg);
        if (TELEM && SIGMA_MODE == 2)
          store_wrow_regs<T, true, 1>(d_lds, creg);
        __syncthreads();
        // prefetch the next round's weights while the MFMAs run
        int rn = r, ckn = ck + BK;
        if (ckn >= p.Kr) { ckn = 0; ++rn; }
        bool more = true;
        if (t + 1 == ROUNDS) {
          rn = 0; ckn = 0;
          more = (m0 + MSUB * BM) < p.MI;  // wraps for the next m-tile pass
        }
        if (more) {
          if (WANT_Y) load_wrow_regs(breg, wq, g, p, n0, rn, ckn);
          if (SIGMA_MODE > 0) load_wrow_regs(creg, wraw, g, p, n0, rn, ckn);
        }
        typename Mma<T>::frag bfrag[2], sfrag[2], tfrag[2];
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          int brow = wn * 32 + fn * 16 + (lane & 15);
          if (WANT_Y) bfrag[fn] = Mma<T>::load(b_lds, brow, lane);
          if (SIGMA_MODE > 0) sfrag[fn] = Mma<T>::load(c_lds, brow, lane);
          if (TELEM && SIGMA_MODE == 2)
            tfrag[fn] = Mma<T>::load(d_lds, brow, lane);
        }
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms) {
          if (ms >= nsub) break;
#pragma unroll
          for (int fm = 0; fm < 2; ++fm) {
            // per-lane patch fragment: 8 contiguous (s,c) at filter row r;
            // span start from the hoisted base (no divisions in the loop)
            int ih = a_ohs[ms][fm] + r;
            int64_t off = zero_off;
            if (ih >= 0 && ih < g.H)
              off = (int64_t)(a_base[ms][fm] + r * rowpitch + ck) * EB;
            auto a = Mma<T>::load_span(patch + off, lane);
#pragma unroll
            for (int fn = 0; fn < 2; ++fn) {
              if (WANT_Y) Mma<T>::mma(a, bfrag[fn], acc[ms][fm][fn]);
              if (SIGMA_MODE > 0) Mma<T>::mma(a, sfrag[fn], sacc[ms][fm][fn]);
              if (TELEM && SIGMA_MODE == 2)
                Mma<T>::mma(a, tfrag[fn], tacc[ms][fm][fn]);
            }
          }
        }
        __syncthreads();
      }
      ck += BK;
      if (ck >= p.Kr) { ck = 0; ++r; }
    }

    // epilogue for the resident m-subtiles
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms) {
      if (ms >= nsub) break;
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          int mb_local = m0 + ms * BM + wm * 32 + fm * 16 + 4 * (lane >> 4);
          int k = n0 + wn * 32 + fn * 16 + (lane & 15);
          float g4[4];
          if (SIGMA_MODE > 0)
            gauss4(seed,
                   (uint64_t)(((int64_t)n * p.MI + mb_local) * g.K + k), g4);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            int m_local = mb_local + reg;
            if (m_local < p.MI && k < g.K) {
              int64_t m = (int64_t)n * p.MI + m_local;
              float y = WANT_Y ? acc[ms][fm][fn][reg] : 0.0f;
              if (BIAS) y += bias[k];
              float v = y;
              if (SIGMA_MODE > 0) {
                float sig = fmaxf(sacc[ms][fm][fn][reg], 0.0f);
                float noise = g4[reg] * sqrtf(factor * sig);
                v = y + noise;
                if (TELEM) {
                  t_sum_noise += fabsf(noise);
                  t_max_y = fmaxf(t_max_y, y);
                  t_sum_sigma += (SIGMA_MODE == 2) ? tacc[ms][fm][fn][reg]
                                                   : sacc[ms][fm][fn][reg];
                }
              }
              out[m * g.K + k] = from_f32<T>(v);
            }
          }
        }
      }
    }
  }

  if (TELEM && SIGMA_MODE > 0) {
    __shared__ float red[4];
    float s0 = block_sum(t_sum_sigma, red);
    __syncthreads();
    float s1 = block_sum(t_sum_noise, red);
    __syncthreads();
    float m0v = wave_max(t_max_y);
    __shared__ float redm[4];
    if ((threadIdx.x & (WAVE - 1)) == 0) redm[threadIdx.x / WAVE] = m0v;
    __syncthreads();
    if (threadIdx.x == 0) {
      atomicAdd(&telem[0], s0);
      atomicAdd(&telem[1], s1);
      atomic_max_f32(&telem[2],
                     fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3])));
    }
  }
}

// --------------------------------------------------------------------------
// Layer-fitted image-patch tiles: ONE block per image covers every output
// pixel and every output channel, so the image is staged once and no
// block runs a mostly-empty N tile (conv2 dgrad, K = 65, spent half its
// grid on one useful column of 64). The 4 waves are laid out WMS over M
// by 4/WMS over N; a wave owns the 16-row M-fragments  i*WMS + wave%WMS
// (i < MF) and the 16-column N-fragments  j*(4/WMS) + wave/WMS  (j < NF),
// interleaved so that tail and skipped fragments spread over the waves.
// M-fragments stay 16-aligned from pixel 0 and every output element is
// still one chain of 16x16x32 MFMAs in (r, ck) order, so outputs and the
// noise draw are bit-identical to the 64x64 kernel above.
//
// Row skip: a (M-fragment, filter row r) pair whose 16 pixels all fall in
// the vertical zero padding (or past MI) would multiply the zero slot;
// a per-fragment bit mask over r, built wave-uniformly before the round
// loop, skips its MFMAs (its prefetched A read is one broadcast read of
// the zero slot). Mixed fragments keep the per-lane zero-slot path.
//
// The weight tile is single-buffered (two barriers per round): a second
// buffer that saves the trailing barrier was measured and costs the third
// resident block per CU on conv2 dgrad (56 KB vs 50 KB of LDS), 5.1 vs
// 3.5 ms at batch 32768.
// 16-bit dtypes, no telemetry (see patch_tile for the host-side choice).
// --------------------------------------------------------------------------

// Weight tile of NROWS rows (a multiple of 16, so a slot is live for whole
// waves: the guard is wave-uniform). The image is row-padded to NROWS.
template <typename T, int WSLOTS, int NROWS>
DEV_INLINE void load_wtile_regs(T dst[WSLOTS][8], const T* __restrict__ w,
                                const ConvGeom g, const PatchGeom p, int wid,
                                int r, int ck) {
#pragma unroll
  for (int i = 0; i < WSLOTS; ++i) {
    if (wid * WAVE + i * kBlock >= NROWS * 4) continue;
    int idx = threadIdx.x + i * kBlock;
    int row = idx >> 2;
    int seg = idx & 3;
    *(bf16x8*)dst[i] = *(const bf16x8*)(
        w + ((int64_t)row * g.R + r) * p.Krs + ck + seg * 8);
  }
}

template <typename T, int WSLOTS, int NROWS, bool ABS_TRANSFORM,
          int SIGMA_MODE>
DEV_INLINE void store_wtile_regs(char* lds, const T src[WSLOTS][8], int wid) {
#pragma unroll
  for (int i = 0; i < WSLOTS; ++i) {
    if (wid * WAVE + i * kBlock >= NROWS * 4) continue;
    int idx = threadIdx.x + i * kBlock;
    int row = idx >> 2;
    int seg = idx & 3;
    if (!ABS_TRANSFORM) {
      *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) =
          *(const bf16x8*)src[i];
      continue;
    }
    float vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = fabsf(to_f32(src[i][j]));
      if (SIGMA_MODE == 2) v = v * v + v;
      vals[j] = v;
    }
    Mma<T>::store8(lds, row, seg * 8, vals);
  }
}

template <typename T, int SIGMA_MODE, bool BIAS, int WMS, int MF, int NF>
__global__ __launch_bounds__(kBlock)
void conv_fwd_patch_tile_kernel(const T* __restrict__ x,
                                const T* __restrict__ wq,
                                const T* __restrict__ wraw,
                                const float* __restrict__ bias,
                                T* __restrict__ out, ConvGeom g, PatchGeom p,
                                const float* __restrict__ factor_p,
                                uint64_t seed,
                                const int64_t* __restrict__ seed_base =
                                    nullptr) {
  using Frag = typename Mma<T>::frag;
  constexpr int WNS = 4 / WMS;
  constexpr int NROWS = WNS * NF * 16;  // weight rows = N extent of the tile
  constexpr int WSLOTS = (NROWS * 4 + kBlock - 1) / kBlock;
  constexpr int EB = 2;
  constexpr int STR = Mma<T>::STRIDE;
  constexpr int WBUF = NROWS * STR;  // one weight tile
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  const int n = blockIdx.y;  // image

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* patch = smem;  // H * Wp * C_pad elements + one zero span
  const int zero_off = g.H * p.Wp * p.C_pad * EB;
  char* b_lds = smem + zero_off + 128;  // wq tile
  char* c_lds = b_lds + WBUF;           // sigma-weight tile

  // wave-uniform wave index: every fragment guard below is a scalar branch
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int wmi = wid % WMS, wni = wid / WMS;
  const int lane = threadIdx.x & (WAVE - 1);

  const int CHW = (p.Kr + BK - 1) / BK;
  const int ROUNDS = g.R * CHW;
  T breg[WSLOTS][8], creg[WSLOTS][8];
  load_wtile_regs<T, WSLOTS, NROWS>(breg, wq, g, p, wid, 0, 0);
  if (SIGMA_MODE > 0)
    load_wtile_regs<T, WSLOTS, NROWS>(creg, wraw, g, p, wid, 0, 0);

  stage_patch(patch, x, g, p, n);

  f32x4 acc[MF][NF] = {};
  f32x4 sacc[MF][NF] = {};

  // hoisted per-fragment pixel decode (as in the 64x64 kernel) and the
  // wave-uniform mask of filter rows that reach at least one real input
  // row from this fragment
  int a_ohs[MF];    // oh*stride - pad, or INT_MIN/2 when m >= MI
  int a_base[MF];   // ((ohs*Wp + ow*stride) * C_pad) element offset
  unsigned live[MF];
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    int m_local = (i * WMS + wmi) * 16 + (lane & 15);
    if (m_local < p.MI) {
      int ow = m_local % g.OW;
      int oh = m_local / g.OW;
      int ohs = oh * g.stride - g.pad;
      a_ohs[i] = ohs;
      a_base[i] = (ohs * p.Wp + ow * g.stride) * p.C_pad;
    } else {
      a_ohs[i] = INT_MIN / 2;
      a_base[i] = 0;
    }
    unsigned mask = 0;
    for (int r = 0; r < g.R; ++r) {  // host guarantees R <= 32
      int ih = a_ohs[i] + r;
      if (__ballot(ih >= 0 && ih < g.H) != 0) mask |= 1u << r;
    }
    live[i] = __builtin_amdgcn_readfirstlane(mask);
  }
  const int rowpitch = p.Wp * p.C_pad;

  // The patch never changes, so the A fragments of round t+1 are read
  // while round t's MFMAs run and their LDS latency is off the round's
  // critical path. A fully padded (fragment, r) pair reads the zero slot
  // (one broadcast address) and its MFMAs are skipped.
  auto load_a = [&](Frag dst[MF], int r, int ck) {
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      int ih = a_ohs[i] + r;
      int off = zero_off;
      if (ih >= 0 && ih < g.H) off = (a_base[i] + r * rowpitch + ck) * EB;
      dst[i] = Mma<T>::load_span(patch + off, lane);
    }
  };
  Frag afrag[MF], anext[MF] = {};
  __syncthreads();  // patch staged
  load_a(afrag, 0, 0);

  int r = 0, ck = 0;
  for (int t = 0; t < ROUNDS; ++t) {
    store_wtile_regs<T, WSLOTS, NROWS, false, 0>(b_lds, breg, wid);
    if (SIGMA_MODE > 0)
      store_wtile_regs<T, WSLOTS, NROWS, true, SIGMA_MODE>(c_lds, creg, wid);
    __syncthreads();
    int rn = r, ckn = ck + BK;
    if (ckn >= p.Kr) { ckn = 0; ++rn; }
    Frag bfrag[NF], sfrag[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      int brow = (j * WNS + wni) * 16 + (lane & 15);
      bfrag[j] = Mma<T>::load(b_lds, brow, lane);
      if (SIGMA_MODE > 0) sfrag[j] = Mma<T>::load(c_lds, brow, lane);
    }
    // prefetch the next round's weights and A fragments under the MFMAs
    if (t + 1 < ROUNDS) {
      load_wtile_regs<T, WSLOTS, NROWS>(breg, wq, g, p, wid, rn, ckn);
      if (SIGMA_MODE > 0)
        load_wtile_regs<T, WSLOTS, NROWS>(creg, wraw, g, p, wid, rn, ckn);
      load_a(anext, rn, ckn);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      if (!((live[i] >> r) & 1u)) continue;  // wave-uniform row skip
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        Mma<T>::mma(afrag[i], bfrag[j], acc[i][j]);
        if (SIGMA_MODE > 0) Mma<T>::mma(afrag[i], sfrag[j], sacc[i][j]);
      }
    }
    __syncthreads();  // all B reads done before the next round's store
#pragma unroll
    for (int i = 0; i < MF; ++i) afrag[i] = anext[i];
    r = rn;
    ck = ckn;
  }

  // epilogue: the 64x64 kernel's maths on this wave's fragments
#pragma unroll
  for (int i = 0; i < MF; ++i) {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      int mb_local = (i * WMS + wmi) * 16 + 4 * (lane >> 4);
      int k = (j * WNS + wni) * 16 + (lane & 15);
      if (mb_local >= p.MI || k >= g.K) continue;
      float g4[4];
      if (SIGMA_MODE > 0)
        gauss4(seed, (uint64_t)(((int64_t)n * p.MI + mb_local) * g.K + k), g4);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int m_local = mb_local + reg;
        if (m_local < p.MI) {
          int64_t m = (int64_t)n * p.MI + m_local;
          float y = acc[i][j][reg];
          if (BIAS) y += bias[k];
          float v = y;
          if (SIGMA_MODE > 0) {
            float sig = fmaxf(sacc[i][j][reg], 0.0f);
            float noise = g4[reg] * sqrtf(factor * sig);
            v = y + noise;
          }
          out[m * g.K + k] = from_f32<T>(v);
        }
      }
    }
  }
}

inline bool patch_eligible(const ConvGeom& g, int elem_bytes) {
  int c_pad = (g.C + 7) & ~7;
  int wp = g.W + 2 * g.pad;
  size_t patch_bytes = (size_t)g.H * wp * c_pad * elem_bytes + 128;
  return g.R * g.S > 1 && g.C > 8 && patch_bytes <= 96 * 1024;
}

// Route of the fused noisy conv. The one place the choice is made:
// conv_fwd_fused / sigma_noise_conv dispatch on it and conv_fused_route
// reports it. The two Col routes differ only in the GEMM that
// linear_route picks for the im2col matrix.
enum class ConvRoute { Patch, ColSmallK, ColGemm, Stream };

// width of the flat im2col matrix (see im2col_materialize)
inline int col_width(const ConvGeom& g) {
  int rsc = g.R * g.S * g.C;
  return ((g.C & 7) == 0) ? rsc : ((rsc + 31) & ~31);
}

inline ConvRoute conv_route(const ConvGeom& g, int elem_bytes) {
  if (patch_eligible(g, elem_bytes)) return ConvRoute::Patch;
  if (g.flat)
    return linear_route(col_width(g), g.K, elem_bytes) == LinearRoute::SmallK
               ? ConvRoute::ColSmallK
               : ConvRoute::ColGemm;
  return ConvRoute::Stream;
}

// Block tile of the patch route. The one place the choice is made:
// conv_fwd_fused_patch_impl launches by it and conv_patch_tile reports it.
//   Plain  (SIGMA_MODE 0, one accumulator set): K <= 80, MI <= 256 ->
//          4 waves over M, each up to 4 M-fragments x all <= 5 N-fragments
//          (conv2 dgrad: 13 x 5, 8.3 -> 3.5 ms at batch 32768)
//   Noisy  (SIGMA_MODE 1/2, two accumulator sets, no telemetry):
//          K <= 128, MI <= 112 -> 4 waves over N, each 1 or 2 N-fragments
//          (the N extent is 4 or 8 fragments, zero weight rows past K)
//          x all <= 7 M-fragments (conv2 forward: 7 x 8). Bit-identical
//          but SLOWER than the 64x64 tile on conv2 forward (8.6 vs 6.5 ms),
//          so it runs only under NOISYNET_PATCH_TILE=all.
//   Generic: the 64x64 tile -- everything else, and every layer under
//          NOISYNET_PATCH_TILE=generic. The variable is read per call.
enum class PatchTile { Generic, Plain, Noisy };

struct PatchTileChoice {
  PatchTile kind;
  int mfrag, nfrag;  // 16-row / 16-column fragments the layer needs
  int nf_wave;       // N-fragments per wave (compile-time in the kernel)
  int nrows;         // weight rows the tile stages = its N extent
};

inline PatchTileChoice patch_tile(const ConvGeom& g, int elem_bytes,
                                  int sigma_mode, bool telem, bool want_y) {
  PatchTileChoice c{PatchTile::Generic, 0, 0, 0, 0};
  const char* e = getenv("NOISYNET_PATCH_TILE");
  if (e && strcmp(e, "generic") == 0) return c;
  const bool all = e && strcmp(e, "all") == 0;
  if (elem_bytes != 2 || telem || !want_y || g.R > 32) return c;
  int mi = g.OH * g.OW;
  c.mfrag = (mi + 15) / 16;
  c.nfrag = (g.K + 15) / 16;
  if (sigma_mode == 0 && g.K <= 80 && mi <= 256) {
    c.kind = PatchTile::Plain;  // every wave owns all N-fragments
    c.nf_wave = c.nfrag;
    c.nrows = c.nfrag * 16;
  } else if (all && sigma_mode > 0 && g.K <= 128 && mi <= 112) {
    c.kind = PatchTile::Noisy;  // N-fragments dealt out over the 4 waves
    c.nf_wave = (c.nfrag + 3) / 4;
    c.nrows = 4 * c.nf_wave * 16;
  }
  return c;
}

// pad the raw-[K,R,S,C] weight view to [K,R,S*C_pad] (tiny tensors)
inline torch::Tensor pad_weight_raw(const torch::Tensor& w, int c_pad) {
  auto raw = w.permute({0, 2, 3, 1});  // logical [K,C,R,S] cl -> raw view
  auto padded = at::constant_pad_nd(raw, {0, c_pad - (int)w.size(1)}, 0);
  return padded.contiguous();  // [K, R, S, C_pad]
}

// fully padded weight image for the patch kernel: [k_pad, R, krs] with
// zero rows beyond K and zero column tails beyond S*C_pad, so the
// staging loads need no bounds checks (see load_wrow_regs)
inline torch::Tensor pad_weight_full(const torch::Tensor& w, int c_pad,
                                     int k_pad, int krs) {
  int64_t K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
  auto raw = w.permute({0, 2, 3, 1});  // [K, R, S, C] view
  auto out = torch::zeros({(int64_t)k_pad, R, (int64_t)krs}, w.options());
  auto padded = at::constant_pad_nd(raw, {0, c_pad - C}, 0)
                    .reshape({K, R, S * (int64_t)c_pad});
  out.narrow(0, 0, K).narrow(2, 0, S * (int64_t)c_pad).copy_(padded);
  return out;
}

}  // namespace


namespace {

// Launch of a layer-fitted tile (16-bit T only; the caller checked
// tile.kind != Generic).
template <typename T>
void launch_patch_tile(const PatchTileChoice& tile, const ConvGeom& g,
                       const PatchGeom& p, const torch::Tensor& x,
                       torch::Tensor& out, const torch::Tensor& wq_pad,
                       const torch::Tensor& wraw_pad,
                       const torch::Tensor& bias_f, bool has_bias,
                       const torch::Tensor& factor_f, int64_t seed,
                       int64_t sigma_mode, int k_pad) {
  if constexpr (sizeof(T) == 2) {
    // one block per image; patch + one weight tile per accumulator set
    size_t tlds = (size_t)g.H * p.Wp * p.C_pad * 2 + 128
                  + (size_t)(sigma_mode > 0 ? 2 : 1) * k_pad * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* wqp = (const T*)wq_pad.data_ptr();
    const T* wrp = (sigma_mode > 0) ? (const T*)wraw_pad.data_ptr() : wqp;
    const float* bp = has_bias ? bias_f.data_ptr<float>() : nullptr;
    auto launch = [&](auto kfn) {
      if (tlds > 64 * 1024)
        hipFuncSetAttribute((const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)tlds);
      hipLaunchKernelGGL(kfn, dim3(1, g.N), dim3(kBlock), tlds, stream,
                         (const T*)x.data_ptr(), wqp, wrp, bp,
                         (T*)out.data_ptr(), g, p,
                         factor_f.data_ptr<float>(), (uint64_t)seed,
                         g_seed_base);
    };
    // <SIGMA_MODE, BIAS, waves over M, M-frags/wave, N-frags/wave>
    auto plain = [&](auto nf) {
      constexpr int NFW = decltype(nf)::value;
      if (has_bias) launch(&conv_fwd_patch_tile_kernel<T, 0, true, 4, 4, NFW>);
      else launch(&conv_fwd_patch_tile_kernel<T, 0, false, 4, 4, NFW>);
    };
    auto noisy = [&](auto sm, auto nf) {
      constexpr int SM = decltype(sm)::value;
      constexpr int NFW = decltype(nf)::value;
      if (has_bias) launch(&conv_fwd_patch_tile_kernel<T, SM, true, 1, 7, NFW>);
      else launch(&conv_fwd_patch_tile_kernel<T, SM, false, 1, 7, NFW>);
    };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using I4 = std::integral_constant<int, 4>;
    using I5 = std::integral_constant<int, 5>;
    if (tile.kind == PatchTile::Plain) {
      switch (tile.nf_wave) {
        case 1: plain(I1{}); break;
        case 2: plain(I2{}); break;
        case 3: plain(I3{}); break;
        case 4: plain(I4{}); break;
        default: plain(I5{}); break;
      }
    } else if (sigma_mode == 1) {
      if (tile.nf_wave == 1) noisy(I1{}, I1{}); else noisy(I1{}, I2{});
    } else {
      if (tile.nf_wave == 1) noisy(I2{}, I1{}); else noisy(I2{}, I2{});
    }
  } else {
    TORCH_CHECK(false, "conv_fwd_patch: layer-fitted tiles are 16-bit only");
  }
}

torch::Tensor pad_cols8(const torch::Tensor& in, int64_t K8);

// NOISYNET_CONV_PAD_SHARE=0 keeps the noisy patch forward on the unpadded
// input (and its backward padding again); read per call.
bool conv_pad_share_enabled() {
  const char* e = getenv("NOISYNET_CONV_PAD_SHARE");
  return e == nullptr || std::string(e) != "0";
}

// Returns {out, telemetry, x_pad}: x_pad is the [N*H*W, C_pad] channel-padded
// copy of a 16-bit input with C % 8 != 0 that the noisy forward ran on (empty
// otherwise); conv_wgrad_patch takes it in place of padding again.
// x_prepadded: the caller already holds that padded copy (bn_act_quant_fwd
// writes it directly). x then gives the logical shape only and is never read;
// the copy is run on as it is and handed back as x_pad.
std::vector<torch::Tensor> conv_fwd_fused_patch_impl(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t seed, bool telem, bool want_y,
    const c10::optional<torch::Tensor>& x_prepadded = c10::nullopt) {
  // the noise-free S0 variant exists with the y accumulator only
  check_sigma_mode(sigma_mode, want_y, "conv_fwd_fused (patch route)");
  const bool prepadded = x_prepadded.has_value() && x_prepadded->numel() > 0;
  if (!prepadded) check_cl(x, "conv_fwd_patch x");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)wraw.size(0), (int)wraw.size(2),
                     (int)wraw.size(3), (int)stride, (int)pad);
  PatchGeom p;
  p.C_pad = (g.C + 7) & ~7;
  p.Wp = g.W + 2 * g.pad;
  p.Kr = g.S * p.C_pad;
  p.Krs = (p.Kr + 31) & ~31;
  p.MI = g.OH * g.OW;
  auto out = torch::empty({g.N, g.K, g.OH, g.OW},
                          x.options().memory_format(at::MemoryFormat::ChannelsLast));
  bool has_bias = bias.numel() > 0;
  torch::Tensor bias_f;
  if (has_bias) bias_f = bias.to(torch::kFloat32).contiguous();
  // telemetry buffer only when requested (steady-state training has
  // telem=false; the zeros+fill launches were ~12 tiny kernels/step)
  auto tele = telem
      ? [&] {
          auto t = torch::zeros({3}, x.options().dtype(torch::kFloat32));
          t[2] = -std::numeric_limits<float>::infinity();
          return t;
        }()
      : torch::empty({0}, x.options().dtype(torch::kFloat32));
  auto factor_f = factor.to(torch::kFloat32).reshape({1}).contiguous();
  // fully padded weight image (rows to the k-tile multiple, columns to
  // round32): staging loads become unconditional 16-B vectors
  const PatchTileChoice tile = patch_tile(g, (int)x.element_size(),
                                          (int)sigma_mode, telem, want_y);
  // noisy forward of a 16-bit input with C % 8 != 0: pad the channels once
  // and stage from the copy with 16-byte vectors (the scalar path pays two
  // divisions per element, once per k-tile). The weight image is laid out
  // for C_pad already, so the LDS patch and the output are bit-identical;
  // the copy goes back to the caller for the weight gradient.
  torch::Tensor x_pad = torch::empty({0}, x.options());
  const bool pad_route = want_y && sigma_mode > 0 && x.element_size() == 2 &&
                         (g.C & 7) != 0 && conv_pad_share_enabled();
  if (prepadded) {
    TORCH_CHECK(pad_route,
                "conv_fwd_fused: a pre-padded input is taken by the noisy "
                "16-bit patch route with C % 8 != 0 only");
    TORCH_CHECK(x_prepadded->dim() == 2 &&
                    x_prepadded->size(0) == (int64_t)g.N * g.H * g.W &&
                    x_prepadded->size(1) == p.C_pad &&
                    x_prepadded->is_contiguous() &&
                    x_prepadded->scalar_type() == x.scalar_type() &&
                    x_prepadded->device() == x.device(),
                "conv_fwd_fused: x_padded must be [N*H*W, round8(C)]");
    x_pad = *x_prepadded;
    x = x_pad;
    g.C = p.C_pad;
  } else if (pad_route) {
    x_pad = pad_cols8(x.permute({0, 2, 3, 1})
                          .reshape({(int64_t)g.N * g.H * g.W, (int64_t)g.C})
                          .contiguous(), p.C_pad);
    x = x_pad;
    g.C = p.C_pad;
  }
  // weight rows follow the N extent of the chosen tile
  int k_pad = tile.kind == PatchTile::Generic ? (g.K + BN - 1) / BN * BN
                                              : tile.nrows;
  auto wq_pad = want_y ? pad_weight_full(wq, p.C_pad, k_pad, p.Krs)
                       : torch::Tensor();
  auto wraw_pad = (sigma_mode > 0)
                      ? pad_weight_full(wraw, p.C_pad, k_pad, p.Krs)
                      : torch::Tensor();
  size_t lds = 0;  // per-dtype, set inside the dispatch
  dim3 grid((g.K + BN - 1) / BN, g.N);
  NN_DISPATCH(x.scalar_type(), "conv_fwd_patch", [&] {
    using T = typename DevT<scalar_t>::type;
    if (tile.kind != PatchTile::Generic) {
      launch_patch_tile<T>(tile, g, p, x, out, wq_pad, wraw_pad, bias_f,
                           has_bias, factor_f, seed, sigma_mode, k_pad);
      return;
    }
    lds = (size_t)g.H * p.Wp * p.C_pad * sizeof(T) + 128
          + (size_t)3 * BN * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = want_y ? (const T*)wq_pad.data_ptr()
                          : (const T*)wraw_pad.data_ptr();
    const T* wrp = (sigma_mode > 0) ? (const T*)wraw_pad.data_ptr() : wqp;
    const float* bp = has_bias ? bias_f.data_ptr<float>() : nullptr;
    T* op = (T*)out.data_ptr();
    float* tp = telem ? tele.data_ptr<float>() : nullptr;
    const float* f = factor_f.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    auto launch = [&](auto wy, auto sm, auto tl, auto bi) {
      hipLaunchKernelGGL((conv_fwd_patch_kernel<T, decltype(wy)::value,
                          decltype(sm)::value, decltype(tl)::value,
                          decltype(bi)::value>), grid, dim3(kBlock), lds,
                         stream, xp, wqp, wrp, bp, op, g, p, f, sd, tp, g_seed_base);
    };
    using TT = std::true_type; using FF = std::false_type;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    if (want_y) {
      if (sigma_mode == 0) {
        if (has_bias) launch(TT{}, S0{}, FF{}, TT{});
        else launch(TT{}, S0{}, FF{}, FF{});
      } else if (sigma_mode == 1) {
        if (telem) { if (has_bias) launch(TT{}, S1{}, TT{}, TT{}); else launch(TT{}, S1{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S1{}, FF{}, TT{}); else launch(TT{}, S1{}, FF{}, FF{}); }
      } else {
        if (telem) { if (has_bias) launch(TT{}, S2{}, TT{}, TT{}); else launch(TT{}, S2{}, TT{}, FF{}); }
        else { if (has_bias) launch(TT{}, S2{}, FF{}, TT{}); else launch(TT{}, S2{}, FF{}, FF{}); }
      }
    } else {
      if (sigma_mode == 1) {
        if (telem) launch(FF{}, S1{}, TT{}, FF{}); else launch(FF{}, S1{}, FF{}, FF{});
      } else {
        if (telem) launch(FF{}, S2{}, TT{}, FF{}); else launch(FF{}, S2{}, FF{}, FF{});
      }
    }
  });
  HIP_CHECK_LAST();
  return {out, tele, x_pad};
}

}  // namespace

// defined below (im2col section); used by the flat/small-C fused route
torch::Tensor im2col_materialize(torch::Tensor x, int64_t K, int64_t stride,
                                 int64_t pad, int64_t R, int64_t S);

namespace {

// Flat/small-C convs (C < 16, R*S > 1, e.g. a 5x5 conv over RGB): the
// streaming kernel's per-element (r,s,c) decode gathers scalars; one
// coalesced im2col pass + the 1x1-GEMM fused kernel over the padded
// [M, R*S*c_pad] rows (16-B vectorized staging) is ~3x faster. The
// padded weight columns are zero, so sigma over |W| / |W|^2+|W| and the
// Philox noise index m*K+k are unchanged.
std::vector<torch::Tensor> conv_fwd_fused_col_impl(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t seed, bool telem, bool want_y) {
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)wraw.size(0), (int)wraw.size(2),
                     (int)wraw.size(3), (int)stride, (int)pad);
  int rsc = g.R * g.S * g.C;
  int cols_p = col_width(g);
  // checked here too, before the im2col pass is launched
  check_sigma_mode(sigma_mode,
                   want_y && linear_route(cols_p, g.K, (int64_t)x.element_size())
                                 == LinearRoute::SmallK,
                   "conv_fwd_fused (im2col route)");
  auto col = im2col_materialize(x, g.K, stride, pad, g.R, g.S);  // [M,cols_p]
  TORCH_CHECK(col.size(1) == cols_p, "conv_fwd_fused: im2col width mismatch");
  // flat weight rows: raw [K,R,S,C] view reshaped to [K, R*S*C],
  // column-padded to match col (row padding to the 96-row LDS image
  // happens inside the small-K host so K stays the logical count)
  auto flat_w = [&](const torch::Tensor& w) {
    auto raw = w.permute({0, 2, 3, 1}).reshape({(int64_t)g.K, (int64_t)rsc});
    return at::constant_pad_nd(raw, {0, cols_p - rsc}, 0).contiguous();
  };
  auto wraw_flat = flat_w(wraw);
  auto wq_flat = want_y ? flat_w(wq) : wraw_flat;
  std::vector<torch::Tensor> r;
  if (want_y) {
    r = linear_fwd_fused(col, wq_flat, wraw_flat, bias, sigma_mode, factor,
                         seed, telem);
  } else {
    r = sigma_noise_linear_impl(col, wraw_flat, sigma_mode, factor, seed,
                                telem);
  }
  // [M, K] row-major IS NHWC: reinterpret as a channels_last 4-D view
  auto out = r[0].view({g.N, g.OH, g.OW, g.K}).permute({0, 3, 1, 2});
  return {out, r[1], col};
}

}  // namespace

// Returns {out, telemetry, shared}: the flat im2col matrix when the small-C
// route materialized one (callers pass it back to conv_wgrad_from_col so
// backward skips the materialization), the [N*H*W, C_pad] channel-padded
// input when the noisy patch route made one (for conv_wgrad_patch), else
// empty. With x_padded the caller passes that padded input in: x is then read
// for its (logical, unpadded) shape only and the same tensor comes back as
// the third output; only the patch route takes one.
std::vector<torch::Tensor> conv_fwd_fused(torch::Tensor x, torch::Tensor wq,
                                          torch::Tensor wraw, torch::Tensor bias,
                                          int64_t stride, int64_t pad,
                                          int64_t sigma_mode,
                                          torch::Tensor factor,
                                          int64_t seed, bool telem,
                                          c10::optional<torch::Tensor> x_padded) {
  TORCH_CHECK(x.dim() == 4, "conv_fwd_fused: expected a 4-D x");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)wraw.size(0), (int)wraw.size(2),
                     (int)wraw.size(3), (int)stride, (int)pad);
  auto empty = torch::empty({0}, x.options());
  const bool prepadded = x_padded.has_value() && x_padded->numel() > 0;
  const ConvRoute route = conv_route(g, (int)x.element_size());
  TORCH_CHECK(!prepadded || route == ConvRoute::Patch,
              "conv_fwd_fused: a pre-padded input needs the patch route");
  switch (route) {
    case ConvRoute::Patch: {
      auto r = conv_fwd_fused_patch_impl(x, wq, wraw, bias, stride, pad,
                                         sigma_mode, factor, seed, telem,
                                         true, x_padded);
      return r;
    }
    case ConvRoute::ColSmallK:
    case ConvRoute::ColGemm:
      return conv_fwd_fused_col_impl(x, wq, wraw, bias, stride, pad,
                                     sigma_mode, factor, seed, telem,
                                     /*want_y=*/true);
    case ConvRoute::Stream:
      break;
  }
  auto r = conv_fwd_fused_impl(x, wq, wraw, bias, stride, pad, sigma_mode,
                               factor, seed, telem, /*want_y=*/true);
  return {r[0], r[1], empty};
}

std::vector<torch::Tensor> sigma_noise_conv(torch::Tensor x, torch::Tensor wraw,
                                            int64_t stride, int64_t pad,
                                            int64_t sigma_mode,
                                            torch::Tensor factor,
                                            int64_t seed, bool telem) {
  auto empty_bias = torch::empty({0}, x.options());
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)wraw.size(0), (int)wraw.size(2),
                     (int)wraw.size(3), (int)stride, (int)pad);
  switch (conv_route(g, (int)x.element_size())) {
    case ConvRoute::Patch: {
      auto r = conv_fwd_fused_patch_impl(x, wraw, wraw, empty_bias, stride,
                                         pad, sigma_mode, factor, seed, telem,
                                         false);
      return {r[0], r[1]};
    }
    case ConvRoute::ColSmallK:
    case ConvRoute::ColGemm: {
      auto r = conv_fwd_fused_col_impl(x, wraw, wraw, empty_bias, stride, pad,
                                       sigma_mode, factor, seed, telem,
                                       /*want_y=*/false);
      return {r[0], r[1]};
    }
    case ConvRoute::Stream:
      break;
  }
  return conv_fwd_fused_impl(x, wraw, wraw, empty_bias, stride, pad,
                             sigma_mode, factor, seed, telem, /*want_y=*/false);
}

std::string conv_fused_route(int64_t C, int64_t H, int64_t W, int64_t K,
                             int64_t R, int64_t S, int64_t stride, int64_t pad,
                             int64_t elem_size) {
  // the route does not depend on the batch size
  auto g = make_geom(1, (int)H, (int)W, (int)C, (int)K, (int)R, (int)S,
                     (int)stride, (int)pad);
  switch (conv_route(g, (int)elem_size)) {
    case ConvRoute::Patch: return "patch";
    case ConvRoute::ColSmallK: return "col_smallk";
    case ConvRoute::ColGemm: return "col_gemm";
    case ConvRoute::Stream: break;
  }
  return "stream";
}

// Block tile conv_fwd_fused runs this layer with on the patch route:
// "<M-fragments>x<N-fragments>" for a layer-fitted one-block-per-image
// tile, "generic" for the 64x64 tile, "none" off the patch route.
std::string conv_patch_tile(int64_t C, int64_t H, int64_t W, int64_t K,
                            int64_t R, int64_t S, int64_t stride, int64_t pad,
                            int64_t elem_size, int64_t sigma_mode,
                            bool telem) {
  auto g = make_geom(1, (int)H, (int)W, (int)C, (int)K, (int)R, (int)S,
                     (int)stride, (int)pad);
  if (conv_route(g, (int)elem_size) != ConvRoute::Patch) return "none";
  auto t = patch_tile(g, (int)elem_size, (int)sigma_mode, telem, true);
  if (t.kind == PatchTile::Generic) return "generic";
  return std::to_string(t.mfrag) + "x" + std::to_string(t.nfrag);
}

// ===========================================================================
// im2col materialization + GEMM wgrad.
//
// Wgrad's contraction runs over N*OH*OW with a scattered per-tap input
// gather; on 288 GB HBM it is cheaper to materialize the im2col matrix
// once ([M, R*S*C] padded to a multiple of 8 columns, one coalesced write
// pass) and run the wgrad as a dense GEMM with fully vectorized staging
// than to re-gather per K-chunk. Each thread copies one C-span per
// (pixel, tap), so the row/tap decode happens once per span, not per
// element.
// ===========================================================================

namespace {

template <typename T>
__global__ void im2col_kernel(const T* __restrict__ x, T* __restrict__ out,
                              ConvGeom g, int64_t nspans) {
  // C % 8 == 0 fast path: span = (m, r, s) copies the C channels of one
  // tap as aligned 16-B vectors into the flat row at column rs*C.
  int taps = g.R * g.S;
  for (int64_t span = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       span < nspans; span += (int64_t)gridDim.x * blockDim.x) {
    int rs = (int)(span % taps);
    int64_t m = span / taps;
    int s = rs % g.S;
    int r = rs / g.S;
    int64_t t = m;
    int ow = (int)(t % g.OW);
    t /= g.OW;
    int oh = (int)(t % g.OH);
    t /= g.OH;
    int n = (int)t;
    int ih = oh * g.stride - g.pad + r;
    int iw = ow * g.stride - g.pad + s;
    T* dst = out + (m * taps + rs) * (int64_t)g.C;
    bool inb = (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W);
    const T* src = inb ? x + (((int64_t)n * g.H + ih) * g.W + iw) * g.C
                       : nullptr;
    if (sizeof(T) == 2) {
      for (int c0 = 0; c0 < g.C; c0 += 8) {
        bf16x8 v;
        if (inb) {
          v = *(const bf16x8*)(src + c0);
        } else {
          v = bf16x8{};
        }
        *(bf16x8*)(dst + c0) = v;
      }
    } else {
      for (int c = 0; c < g.C; ++c)
        dst[c] = inb ? src[c] : from_f32<T>(0.0f);
    }
  }
}

// Compile-time (C, S) variant: the % / / decode folds to multiply-shift
// sequences, so there is no LDS table (whose strided reads were 8-way
// bank-conflicted) and no per-block setup. Instantiated for the common
// small-C shapes; the generic table kernel below covers the rest.
template <typename T, int C, int S>
__global__ void im2col_flat_tmpl_kernel(const T* __restrict__ x,
                                        T* __restrict__ out, ConvGeom g,
                                        int cols_p, int64_t nchunks_total) {
  int nchunks = cols_p >> 3;
  int rsc = g.R * g.S * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < nchunks_total; idx += (int64_t)gridDim.x * blockDim.x) {
    int seg = (int)(idx % nchunks);
    int64_t m = idx / nchunks;
    int64_t t = m;
    int ow = (int)(t % g.OW);
    t /= g.OW;
    int oh = (int)(t % g.OH);
    t /= g.OH;
    int n = (int)t;
    int oh0 = oh * g.stride - g.pad;
    int ow0 = ow * g.stride - g.pad;
    const T* xn = x + ((int64_t)n * g.H + oh0) * g.W * g.C + ow0 * g.C;
    T vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int k = seg * 8 + j;
      float v = 0.0f;
      if (k < rsc) {
        int c = k % C;       // constexpr divisor -> mul/shift
        int rs = k / C;
        int ss = rs % S;
        int r = rs / S;
        int ih = oh0 + r;
        int iw = ow0 + ss;
        if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          v = to_f32(xn[(r * g.W + ss) * g.C + c]);
      }
      vals[j] = from_f32<T>(v);
    }
    T* dst = out + m * cols_p + seg * 8;
    if (sizeof(T) == 2) {
      *(bf16x8*)dst = *(bf16x8*)vals;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = vals[j];
    }
  }
}

// C % 8 != 0 (small-C convs): flat row of R*S*C columns padded to a
// multiple of 8; each thread fills one aligned 8-column chunk. The
// (r, s, c) decode of each column (two integer divisions) is computed
// ONCE PER BLOCK into an LDS table -- the per-element version of this
// kernel spent ~90% of its time in the div/mod chain (763 us/step for a
// [1.6M, 80] materialization whose traffic floor is ~40 us).
template <typename T>
__global__ void im2col_flat_kernel(const T* __restrict__ x,
                                   T* __restrict__ out, ConvGeom g,
                                   int cols_p, int64_t nchunks_total,
                                   uint64_t cmul, int cshift, uint64_t smul,
                                   int sshift) {
  // (r, s, c) decode via host-computed magic-number division (the LDS
  // table variant was 8-way bank-conflicted; real division was worse)
  int nchunks = cols_p >> 3;
  int rsc = g.R * g.S * g.C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < nchunks_total; idx += (int64_t)gridDim.x * blockDim.x) {
    int seg = (int)(idx % nchunks);
    int64_t m = idx / nchunks;
    int64_t t = m;
    int ow = (int)(t % g.OW);
    t /= g.OW;
    int oh = (int)(t % g.OH);
    t /= g.OH;
    int n = (int)t;
    int oh0 = oh * g.stride - g.pad;
    int ow0 = ow * g.stride - g.pad;
    const T* xn = x + ((int64_t)n * g.H + oh0) * g.W * g.C + ow0 * g.C;
    T vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int k = seg * 8 + j;
      float v = 0.0f;
      if (k < rsc) {
        // 64-bit multiplier: for divisors just above a power of two the
        // magic constant needs 33 bits; k < cols_p << 2^20 so the product
        // stays well under 2^64
        int rs = (int)(((uint64_t)k * cmul) >> (32 + cshift));
        int c = k - rs * g.C;
        int r = (int)(((uint64_t)rs * smul) >> (32 + sshift));
        int ss = rs - r * g.S;
        int ih = oh0 + r;
        int iw = ow0 + ss;
        if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
          v = to_f32(xn[(r * g.W + ss) * g.C + c]);
      }
      vals[j] = from_f32<T>(v);
    }
    T* dst = out + m * cols_p + seg * 8;
    if (sizeof(T) == 2) {
      *(bf16x8*)dst = *(bf16x8*)vals;  // raw 16 B
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = vals[j];
    }
  }
}

// one-pass column pad: out[m, 0:K] = in[m, 0:K], out[m, K:K8] = 0.
// (at::constant_pad_nd fills the WHOLE output then copies -- two full
// passes, ~0.55 ms at [1.6M, 65->72]; this writes each chunk once.)
template <typename T>
__global__ void pad_cols_kernel(const T* __restrict__ in, T* __restrict__ out,
                                int64_t nchunks_total, int nchunks, int K) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < nchunks_total; idx += (int64_t)gridDim.x * blockDim.x) {
    int seg = (int)(idx % nchunks);
    int64_t m = idx / nchunks;
    const T* src = in + m * K + seg * 8;
    int base = seg * 8;
    T vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      vals[j] = (base + j < K) ? src[j] : from_f32<T>(0.0f);
    T* dst = out + (m * (int64_t)nchunks + seg) * 8;
    if (sizeof(T) == 2) {
      *(bf16x8*)dst = *(bf16x8*)vals;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = vals[j];
    }
  }
}

// LDS-staged variant for odd K (16-bit): an odd row stride makes every
// direct row load 2-B-misaligned, so the simple kernel issued 8 scalar
// loads per output chunk (66% instruction-wait, 5x off bandwidth).
// Here each block copies a 256-row slab: the slab's FLAT source range is
// read with aligned 16-B loads into LDS, then rows are written out of LDS
// (LDS has no vector-alignment constraint) as aligned 16-B stores.
template <typename T>
__global__ void pad_cols_lds_kernel(const T* __restrict__ in,
                                    T* __restrict__ out, int64_t M,
                                    int nchunks, int K) {
  constexpr int ROWS = 256;
  extern __shared__ __attribute__((aligned(16))) char praw[];
  T* slab = (T*)praw;  // ROWS * K elements
  for (int64_t r0 = (int64_t)blockIdx.x * ROWS; r0 < M;
       r0 += (int64_t)gridDim.x * ROWS) {
    int64_t e0 = r0 * K;                       // slab's flat element range
    int64_t e1 = (r0 + ROWS < M ? r0 + ROWS : M) * K;
    // aligned 16-B window covering [e0, e1)
    int64_t a0 = e0 & ~(int64_t)7;
    for (int64_t e = a0 + (int64_t)threadIdx.x * 8; e < e1; e += 256 * 8) {
      T vals[8];
      if (e >= e0 && e + 8 <= e1) {
        *(bf16x8*)vals = *(const bf16x8*)(in + e);
#pragma unroll
        for (int j = 0; j < 8; ++j) slab[e - e0 + j] = vals[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int64_t ee = e + j;
          if (ee >= e0 && ee < e1) slab[ee - e0] = in[ee];
        }
      }
    }
    __syncthreads();
    int64_t rows_here = (e1 - e0) / K;
    int64_t total = rows_here * nchunks;  // output 8-chunks in this slab
    for (int64_t t = threadIdx.x; t < total; t += 256) {
      int64_t lr = t / nchunks;
      int seg = (int)(t - lr * nchunks);
      int base = seg * 8;
      T vals[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        vals[j] = (base + j < K) ? slab[lr * K + base + j]
                                 : from_f32<T>(0.0f);
      *(bf16x8*)(out + ((r0 + lr) * (int64_t)nchunks + seg) * 8) =
          *(bf16x8*)vals;
    }
    __syncthreads();
  }
}

torch::Tensor pad_cols8(const torch::Tensor& in, int64_t K8) {
  TORCH_CHECK(in.dim() == 2 && in.is_contiguous());
  int64_t M = in.size(0);
  int K = (int)in.size(1);
  auto out = torch::empty({M, K8}, in.options());
  int nchunks = (int)(K8 >> 3);
  int64_t total = M * nchunks;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  NN_DISPATCH(in.scalar_type(), "pad_cols8", [&] {
    using T = typename DevT<scalar_t>::type;
    size_t slab = (size_t)256 * K * sizeof(T);
    if (sizeof(T) == 2 && slab <= 64 * 1024) {
      int lblocks = (int)std::min<int64_t>((M + 255) / 256, 2048);
      hipLaunchKernelGGL((pad_cols_lds_kernel<T>), dim3(lblocks), dim3(256),
                         slab, c10::hip::getCurrentHIPStream(),
                         (const T*)in.data_ptr(), (T*)out.data_ptr(), M,
                         nchunks, K);
    } else {
      hipLaunchKernelGGL((pad_cols_kernel<T>), dim3(blocks), dim3(256), 0,
                         c10::hip::getCurrentHIPStream(),
                         (const T*)in.data_ptr(), (T*)out.data_ptr(), total,
                         nchunks, K);
    }
  });
  HIP_CHECK_LAST();
  return out;
}

}  // namespace

// Materialize the im2col matrix [M, cols_p] with the FLAT column layout:
// column k = flattened (r, s, c), row padded with zeros to cols_p =
// round8(R*S*C). (For C % 8 == 0 that equals the per-tap layout.)
// Exposed for testing.
torch::Tensor im2col_materialize(torch::Tensor x, int64_t K, int64_t stride,
                                 int64_t pad, int64_t R, int64_t S) {
  check_cl(x, "im2col x");
  auto g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                     (int)x.size(1), (int)K, (int)R, (int)S, (int)stride,
                     (int)pad);
  int taps = g.R * g.S;
  // small-C (flat-kernel) path: round32 so every 32-wide contraction
  // chunk of the consumers (small-K fused GEMM, wgrad stagers) is fully
  // in-bounds -- bounds-checked tails compile to serialized exec-masked
  // scalar loads. The aligned span path writes exactly taps*C columns
  // (no zeroed tail), so it keeps the tight width.
  int cols_p = ((g.C & 7) == 0) ? taps * g.C : ((taps * g.C + 31) & ~31);
  auto col = torch::empty({g.M, cols_p}, x.options());
  NN_DISPATCH(x.scalar_type(), "im2col", [&] {
    using T = typename DevT<scalar_t>::type;
    auto stream = c10::hip::getCurrentHIPStream();
    if ((g.C & 7) == 0) {
      int64_t nspans = g.M * taps;
      int blocks = (int)std::min<int64_t>((nspans + 255) / 256, 8192);
      hipLaunchKernelGGL((im2col_kernel<T>), dim3(blocks), dim3(256), 0,
                         stream, (const T*)x.data_ptr(), (T*)col.data_ptr(),
                         g, nspans);
    } else {
      int64_t nchunks_total = g.M * (cols_p >> 3);
      int blocks = (int)std::min<int64_t>((nchunks_total + 255) / 256, 8192);
      if (g.C == 3 && g.S == 5) {
        hipLaunchKernelGGL((im2col_flat_tmpl_kernel<T, 3, 5>), dim3(blocks),
                           dim3(256), 0, stream, (const T*)x.data_ptr(),
                           (T*)col.data_ptr(), g, cols_p, nchunks_total);
      } else if (g.C == 3 && g.S == 3) {
        hipLaunchKernelGGL((im2col_flat_tmpl_kernel<T, 3, 3>), dim3(blocks),
                           dim3(256), 0, stream, (const T*)x.data_ptr(),
                           (T*)col.data_ptr(), g, cols_p, nchunks_total);
      } else {
        auto magic = [](uint32_t d, uint64_t& mul, int& sh) {
          sh = 0;
          while ((1u << sh) < d) ++sh;
          mul = (uint64_t)(((__uint128_t)1 << (32 + sh)) / d) + 1;
        };
        uint64_t cmul, smul;
        int cshift, sshift;
        magic((uint32_t)g.C, cmul, cshift);
        magic((uint32_t)g.S, smul, sshift);
        hipLaunchKernelGGL((im2col_flat_kernel<T>), dim3(blocks), dim3(256),
                           0, stream, (const T*)x.data_ptr(),
                           (T*)col.data_ptr(), g, cols_p, nchunks_total,
                           cmul, cshift, smul, sshift);
      }
    }
  });
  HIP_CHECK_LAST();
  return col;
}

torch::Tensor conv_wgrad_from_col(torch::Tensor gy, torch::Tensor col,
                                  int64_t C, int64_t R, int64_t S);

// conv wgrad through materialized im2col (called from Python when the
// buffer fits; falls back to conv_wgrad otherwise).
torch::Tensor conv_wgrad_im2col(torch::Tensor gy, torch::Tensor x,
                                int64_t stride, int64_t pad, int64_t R,
                                int64_t S) {
  check_cl(gy, "conv_wgrad_im2col gy");
  check_cl(x, "conv_wgrad_im2col x");
  auto col = im2col_materialize(x, gy.size(1), stride, pad, R, S);
  return conv_wgrad_from_col(gy, col, x.size(1), R, S);
}

// Which kernel conv_wgrad_patch runs for a layer: "window"
// (conv_wgrad_window_kernel) or "legacy" (conv_wgrad_patch_kernel).
// NOISYNET_WGRAD_PATCH=legacy forces the latter; read per call. The batch
// size is not part of the rule (beyond 2^31 output pixels the call itself
// takes the legacy kernel).
std::string conv_wgrad_route(int64_t C, int64_t H, int64_t W, int64_t K,
                             int64_t R, int64_t S, int64_t stride,
                             int64_t pad, int64_t elem_size) {
  if (ww_forced_legacy()) return "legacy";
  return ww_plan(1, C, H, W, K, R, S, stride, pad, elem_size, nullptr)
             ? "window" : "legacy";
}

// Patch wgrad: no materialized im2col (see conv_wgrad_patch_kernel and
// conv_wgrad_window_kernel). 16-bit dtypes; any stride/pad.
torch::Tensor conv_wgrad_patch(torch::Tensor gy, torch::Tensor x,
                               int64_t stride, int64_t pad, int64_t R,
                               int64_t S,
                               c10::optional<torch::Tensor> x_padded) {
  check_cl(gy, "conv_wgrad_patch gy");
  // with x_padded, x gives the shape only and may be any 4-D tensor (the
  // fused BN/quantise route passes a strided view of the padded buffer)
  const bool have_xp = x_padded.has_value() && x_padded->numel() > 0;
  if (have_xp) {
    TORCH_CHECK(x.dim() == 4, "conv_wgrad_patch x: expected a 4-D tensor");
  } else {
    check_cl(x, "conv_wgrad_patch x");
  }
  TORCH_CHECK(x.element_size() == 2, "conv_wgrad_patch: 16-bit only");
  int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int64_t K = gy.size(1), OH = gy.size(2), OW = gy.size(3);
  int64_t M = N * OH * OW;
  int64_t Cp = (C + 7) & ~7;
  int64_t CRSp = R * S * Cp;

  // raw NHWC views (zero-copy for channels_last)
  torch::Tensor xp;
  if (have_xp) {
    // the forward's channel-padded copy of x
    TORCH_CHECK(x_padded->dim() == 2 && x_padded->size(0) == N * H * W &&
                    x_padded->size(1) == Cp && x_padded->is_contiguous() &&
                    x_padded->scalar_type() == x.scalar_type() &&
                    x_padded->device() == x.device(),
                "conv_wgrad_patch: x_padded must be [N*H*W, round8(C)]");
    xp = *x_padded;
  } else {
    auto x2 = x.permute({0, 2, 3, 1}).reshape({N * H * W, C});
    xp = (Cp == C) ? x2.contiguous() : pad_cols8(x2.contiguous(), Cp);
  }
  auto gy2 = gy.permute({0, 2, 3, 1}).reshape({M, K});
  int64_t Kp = (K + 7) & ~7;
  torch::Tensor gyp = (Kp == K) ? gy2.contiguous()
                                : pad_cols8(gy2.contiguous(), Kp);

  int ctiles = (int)((CRSp + 127) / 128);
  int ktiles = (int)((Kp + 127) / 128);
  int64_t mtotal = (M + WG_BK - 1) / WG_BK;
  int64_t target_z = std::max<int64_t>(1, 2048 / std::max(1, ctiles * ktiles));
  int chunks = (int)((mtotal + target_z - 1) / target_z);
  int mslices = (int)((mtotal + chunks - 1) / chunks);
  dim3 grid(ctiles, ktiles, mslices);
  size_t lds = (size_t)256 * WG_LSTR;
  auto parts = torch::empty({(int64_t)mslices, Kp, CRSp},
                            x.options().dtype(torch::kFloat32));
  // the m-slices above are the legacy tile's whatever kernel runs: every
  // output element keeps its accumulation chain, so both routes are
  // bit-identical
  WinGeom wg;
  const bool window = !ww_forced_legacy() &&
                      ww_plan(N, C, H, W, K, R, S, stride, pad,
                              x.element_size(), &wg);
  if (window) {
  NN_DISPATCH(gy.scalar_type(), "conv_wgrad_window", [&] {
    using T = typename DevT<scalar_t>::type;
    if constexpr (sizeof(T) == 2) {
      dim3 wgrid((unsigned)(R * wg.ncolblk), ktiles, mslices);
      size_t wlds = (size_t)WW_GY_BYTES + WW_TAB_BYTES +
                    (size_t)(wg.nslots + 1) * wg.slot_bytes;
      auto* kfn = &conv_wgrad_window_kernel<T>;
      if (wlds > 64 * 1024)
        hipFuncSetAttribute((const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)wlds);
      hipLaunchKernelGGL(kfn, wgrid, dim3(WW_THREADS), wlds,
                         c10::hip::getCurrentHIPStream(),
                         (const T*)gyp.data_ptr(), (const T*)xp.data_ptr(),
                         parts.data_ptr<float>(), (int)M, wg, chunks);
    }
  });
  } else {
  NN_DISPATCH(gy.scalar_type(), "conv_wgrad_patch", [&] {
    using T = typename DevT<scalar_t>::type;
    auto* kfn = &conv_wgrad_patch_kernel<T>;
    if (lds > 64 * 1024)
      hipFuncSetAttribute((const void*)kfn,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds);
    hipLaunchKernelGGL(kfn, grid, dim3(kBlock), lds,
                       c10::hip::getCurrentHIPStream(),
                       (const T*)gyp.data_ptr(), (const T*)xp.data_ptr(),
                       parts.data_ptr<float>(), M, (int)Kp, (int)H, (int)W,
                       (int)OH, (int)OW, (int)S, (int)Cp, (int)CRSp,
                       (int)stride, (int)pad, chunks);
  });
  }
  HIP_CHECK_LAST();
  auto dw = parts.sum(0).narrow(0, 0, K)
                .view({K, R, S, Cp}).narrow(3, 0, C)
                .permute({0, 3, 1, 2})
                .contiguous(at::MemoryFormat::ChannelsLast);
  return dw.to(x.scalar_type());
}

// wgrad when the flat im2col matrix already exists (shared from the
// fused forward's col route -- the input does not change between the
// forward and its backward, so the materialization is paid once).
torch::Tensor conv_wgrad_from_col(torch::Tensor gy, torch::Tensor col,
                                  int64_t C, int64_t R, int64_t S) {
  check_cl(gy, "conv_wgrad_from_col gy");
  TORCH_CHECK(col.dim() == 2 && col.is_contiguous());
  int64_t M = col.size(0);
  int64_t cols_p = col.size(1);
  int64_t K = gy.size(1);
  int64_t rsc = R * S * C;
  TORCH_CHECK((int64_t)gy.size(0) * gy.size(2) * gy.size(3) == M);

  // dw[k, cols_p] = gy^T @ col. Long contractions (M >= 64k) favor the
  // custom split-M kernel (swizzled transposed staging: conv1 0.29 ms vs
  // 1.98 blas; conv2 0.77 vs 0.86); short ones (fc layers) hipBLASLt.
  auto gy2 = gy.permute({0, 2, 3, 1}).reshape({M, K});  // raw view, free
  torch::Tensor dw_flat;
  if (M >= 65536) {
    int64_t K8 = (K + 7) & ~7;
    if (K8 != K && gy.scalar_type() != torch::kFloat32) {
      // odd K (e.g. 65 output channels) leaves gy rows 2-byte-misaligned,
      // forcing scalar staging loads; one zero-pad pass restores 16-B
      // vector loads (the extra dw rows are sliced off below)
      auto gy2p = pad_cols8(gy2.contiguous(), K8);
      dw_flat = linear_wgrad(gy2p, col).narrow(0, 0, K);
    } else {
      dw_flat = linear_wgrad(gy2, col);                     // [K, cols_p]
    }
  } else {
    dw_flat = at::matmul(gy2.t(), col).to(col.scalar_type());
  }
  // un-pad the flat row: [K, cols_p] -> [K, R*S*C] -> logical [K,C,R,S] cl
  auto dw = dw_flat.narrow(1, 0, rsc)
                .view({K, R, S, C})
                .permute({0, 3, 1, 2})
                .contiguous(at::MemoryFormat::ChannelsLast);
  return dw;
}
