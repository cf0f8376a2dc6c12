// What the crossbar kernels (xbar_fwd.hip, xbar_serial.hip, xbar_cells.hip)
// share: the staging of a k-step, the per-partial "noise, then ADC" stage,
// the code-to-digit derivation, the output tail with its telemetry
// reduction, and the host-side prelude, dispatch and conv geometry.
//
// Every kernel has the 64x64 tile / 4 waves in a 2x2 grid / BK = 32 structure
// of conv_fwd_kernel, keeps its own main loop and accumulators, and calls the
// stages below; each stage has this one definition.
#pragma once

#include <c10/hip/HIPStream.h>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>
#include "mfma_tile.h"

namespace {

// The output pixel a thread stages (fixed for the whole contraction) and the
// (r, s, c) position of the first of its 8 crossbar rows in the current
// k-step, advanced by 32 rows per step without a division.
struct XbarRow {
  bool live;        // pixel inside M
  int img, ih0, iw0;
  int r, s, c;
};

DEV_INLINE void xbar_row_advance(XbarRow& p, const ConvGeom& g, int rows) {
  p.c += rows;
  while (p.c >= g.C) {
    p.c -= g.C;
    if (++p.s == g.S) {
      p.s = 0;
      ++p.r;
    }
  }
}

// the output pixel this thread stages, decomposed once, and where its first
// 8-row span starts
DEV_INLINE XbarRow xbar_row_init(const ConvGeom& g, int64_t m0) {
  XbarRow xr;
  int64_t sm = m0 + (threadIdx.x >> 2);
  xr.live = sm < g.M;
  int oh = 0, ow = 0;
  xr.img = 0;
  if (xr.live) {
    int64_t t = sm;
    ow = (int)(t % g.OW); t /= g.OW;
    oh = (int)(t % g.OH); t /= g.OH;
    xr.img = (int)t;
  }
  xr.ih0 = oh * g.stride - g.pad;
  xr.iw0 = ow * g.stride - g.pad;
  xr.r = xr.s = xr.c = 0;
  xbar_row_advance(xr, g, (threadIdx.x & 3) * 8);
  return xr;
}

// One thread's share of a k-step, held in registers between its global loads
// and its LDS stores so the next step's loads fly under this step's MFMAs:
// 8 activations, 8 wq and 8 w_raw elements.
template <typename T>
struct XbarRegs {
  alignas(16) T x[8];
  alignas(16) T q[8];
  alignas(16) T w[8];
};

// activations: 8 consecutive crossbar rows from (r, s, c) on of the thread's
// output pixel. A span inside one filter tap is 16 contiguous bytes for a
// 16-bit dtype: one load (memcpy form, since for C % 8 != 0 the address is
// only element-aligned). A span that straddles taps, or runs past the last
// row (r reaches R), walks element by element; padding positions are zeros.
template <typename T>
DEV_INLINE void xbar_load_x(T (&v)[8], const T* __restrict__ x,
                            const ConvGeom& g, const XbarRow& p) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(0.0f);
  if (!(p.live && p.r < g.R)) return;
  if (p.c + 8 <= g.C) {
    int ih = p.ih0 + p.r, iw = p.iw0 + p.s;
    if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
      const T* px = x + (((int64_t)p.img * g.H + ih) * g.W + iw) * g.C + p.c;
      if (sizeof(T) == 2) {
        __builtin_memcpy(v, px, 16);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = px[j];
      }
    }
  } else {
    int r = p.r, s = p.s, c = p.c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int ih = p.ih0 + r, iw = p.iw0 + s;
      if (r < g.R && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
        v[j] = x[(((int64_t)p.img * g.H + ih) * g.W + iw) * g.C + c];
      if (++c == g.C) {
        c = 0;
        if (++s == g.S) {
          s = 0;
          ++r;
        }
      }
    }
  }
}

// weights from the [K, pitch] row matrices. For 16-bit dtypes the host pads
// rows with zeros to pitch % 8 == 0, so every 8-span is one aligned 16-byte
// load or lies wholly past the row.
template <typename T, int SIGMA_MODE>
DEV_INLINE void xbar_load_w(T (&q)[8], T (&w)[8], const T* __restrict__ wq,
                            const T* __restrict__ wraw, int K, int n0, int ck,
                            int nrows, int pitch) {
  int k = n0 + (threadIdx.x >> 2);
  int c0 = ck + (threadIdx.x & 3) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    q[j] = from_f32<T>(0.0f);
    w[j] = from_f32<T>(0.0f);
  }
  if (k >= K) return;
  const T* pq = wq + (int64_t)k * pitch + c0;
  const T* pr = wraw + (int64_t)k * pitch + c0;
  if (sizeof(T) == 2 && (pitch & 7) == 0) {
    if (c0 + 8 <= pitch) {
      *(bf16x8*)q = *(const bf16x8*)pq;
      if (SIGMA_MODE > 0) *(bf16x8*)w = *(const bf16x8*)pr;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c0 + j < nrows) {
        q[j] = pq[j];
        if (SIGMA_MODE > 0) w[j] = pr[j];
      }
    }
  }
}

template <typename T>
DEV_INLINE void xbar_put8(char* lds, int row, int seg, const T (&v)[8]) {
  if (sizeof(T) == 2) {
    *(bf16x8*)(lds + row * Mma<T>::STRIDE + seg * 16) = *(const bf16x8*)v;
  } else {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = to_f32(v[j]);
    Mma<T>::store8(lds, row, seg * 8, f);
  }
}

// registers -> LDS weight tiles: wq as it is, f(|w_raw|) and (telemetry with
// abs2) |w_raw| derived from the ONE raw-weight load. row = threadIdx.x >> 2
// and seg = threadIdx.x & 3 are the caller's (derived again in here they cost
// the bit-serial kernel two VGPRs).
template <typename T, int SIGMA_MODE, bool TELEM>
DEV_INLINE void xbar_store_w_tiles(char* b_lds, char* c_lds, char* d_lds,
                                   int row, int seg, const XbarRegs<T>& rg) {
  xbar_put8<T>(b_lds, row, seg, rg.q);
  if (SIGMA_MODE > 0) {
    float a[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = fabsf(to_f32(rg.w[j]));
      v[j] = (SIGMA_MODE == 2) ? a[j] * a[j] + a[j] : a[j];
    }
    Mma<T>::store8(c_lds, row, seg * 8, v);
    if (TELEM && SIGMA_MODE == 2) Mma<T>::store8(d_lds, row, seg * 8, a);
  }
}

// "code once, then one digit per slice": the code of a value on the grid
// lo + code * step, and digit t of it at ``bits`` bits per digit
DEV_INLINE int xbar_code(float v, float lo, float inv_step, float code_max) {
  float c = rintf((v - lo) * inv_step);
  return (int)fminf(fmaxf(c, 0.0f), code_max);
}

DEV_INLINE float xbar_digit(int code, int t, int bits, int mask) {
  return (float)((code >> (t * bits)) & mask);
}

// row of register 0 and column of the lane's part of C/D fragment (fm, fn)
// in wave (wm, wn) of the 2x2 wave grid; the tile row a lane reads for an A
// (wm, fm) or a B (wn, fn) fragment
DEV_INLINE int64_t xbar_frag_m(int64_t m0, int wm, int fm, int lane) {
  return m0 + wm * 32 + fm * 16 + 4 * (lane >> 4);
}

DEV_INLINE int xbar_frag_n(int n0, int wn, int fn, int lane) {
  return n0 + wn * 32 + fn * 16 + (lane & 15);
}

DEV_INLINE int xbar_frag_row(int w, int f, int lane) {
  return w * 32 + f * 16 + (lane & 15);
}

// One partial sum through its column: the noise draw, then the ADC.
//   noise = gz * sqrt(factor * sig)       (sig already clamped at zero)
//   v     = p + noise
//   q     = step * clamp(rint(v * inv_step), -top, top)       bipolar
//         = step * clamp(rint(v * inv_step), 0, top)          UNIPOLAR
// Everything comes back by value and the caller keeps its own telemetry (the
// range test on c.t for t_sat, the max of |c.v|): with the kernel's
// loop-carried accumulators passed in by reference, the bit-sliced telemetry
// instantiations went from 246 VGPRs to 256 + 125 AGPRs; with the range test
// in here and a flag returned, one of them went from 169 to 239.
struct XbarPartial {
  float q;       // the converted partial
  float noise;   // zero with SIGMA_MODE 0
  float v;       // p + noise, what the ADC saw
  float t;       // the ADC's code before clamping (0 with the ADC off)
};

template <int SIGMA_MODE, bool ADC, bool UNIPOLAR>
DEV_INLINE XbarPartial xbar_convert(float p, float sig, float gz, float factor,
                                    float step, float inv_step, float top) {
  XbarPartial c;
  c.noise = 0.0f;
  c.v = p;
  if (SIGMA_MODE > 0) {
    c.noise = gz * sqrtf(factor * sig);
    c.v = p + c.noise;
  }
  c.q = c.v;
  c.t = 0.0f;
  if (ADC) {
    float t = rintf(c.v * inv_step);
    c.t = t;
    if (UNIPOLAR) {
      c.q = step * fminf(fmaxf(t, 0.0f), top);
    } else {
      c.q = step * fminf(fmaxf(t, -top), top);
    }
  }
  return c;
}

// The tail of every kernel: bias (nullptr = none; HAS_BIAS says at compile
// time that it is there, and drops the test), the one rounding to the dtype,
// the stores, and the telemetry block reduction with its atomics.
//   telem[5] = sum sigma_abs, sum |total noise|, max clean y, (unused, see
//   sat_count), max |v|; sat_count = number of saturated partials (exact,
//   64-bit: t_sat is a per-thread count far below 2^24)
// wid, wm, wn and lane are the kernel's own values: derived again in here
// they cost two VGPRs in most instantiations and an occupancy step in some.
template <typename T, int SIGMA_MODE, bool ADC, bool TELEM,
          bool HAS_BIAS = false>
DEV_INLINE void xbar_finish(const f32x4 (&oacc)[2][2], const f32x4 (&ycl)[2][2],
                            const f32x4 (&ntot)[2][2],
                            const float* __restrict__ bias,
                            T* __restrict__ out, const ConvGeom& g, int64_t m0,
                            int n0, int wid, int wm, int wn, int lane,
                            float t_sum_sigma, float t_sat, float t_vmax,
                            float* __restrict__ telem,
                            unsigned long long* __restrict__ sat_count) {
  float t_sum_noise = 0.0f, t_max_y = -INFINITY;
#pragma unroll
  for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
      int64_t mb = xbar_frag_m(m0, wm, fm, lane);
      int n = xbar_frag_n(n0, wn, fn, lane);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int64_t m = mb + reg;
        if (m < g.M && n < g.K) {
          float bv = (HAS_BIAS || bias) ? bias[n] : 0.0f;
          out[m * g.K + n] = from_f32<T>(oacc[fm][fn][reg] + bv);
          if (TELEM) {
            t_sum_noise += fabsf(ntot[fm][fn][reg]);
            t_max_y = fmaxf(t_max_y, ycl[fm][fn][reg] + bv);
          }
        }
      }
    }
  }
  if (TELEM) {
    __shared__ float red[4];
    __shared__ float redm[2][4];
    float s0 = block_sum(t_sum_sigma, red);
    __syncthreads();
    float s1 = block_sum(t_sum_noise, red);
    __syncthreads();
    float s3 = block_sum(t_sat, red);
    float my = wave_max(t_max_y);
    float mv = wave_max(t_vmax);
    if (lane == 0) {
      redm[0][wid] = my;
      redm[1][wid] = mv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (SIGMA_MODE > 0) {
        atomicAdd(&telem[0], s0);
        atomicAdd(&telem[1], s1);
      }
      atomic_max_f32(&telem[2], fmaxf(fmaxf(redm[0][0], redm[0][1]),
                                      fmaxf(redm[0][2], redm[0][3])));
      if (ADC) atomicAdd(sat_count, (unsigned long long)(s3 + 0.5f));
      atomic_max_f32(&telem[4], fmaxf(fmaxf(redm[1][0], redm[1][1]),
                                      fmaxf(redm[1][2], redm[1][3])));
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

inline void check_xbar_args(int64_t sigma_mode, int64_t xbar_rows,
                            int64_t adc_bits, const torch::Tensor& adc,
                            const torch::Tensor& x, const char* who) {
  check_sigma_mode(sigma_mode, true, who);
  TORCH_CHECK(xbar_rows > 0 && xbar_rows % BK == 0, who,
              ": xbar_rows must be a positive multiple of ", BK, ", got ",
              xbar_rows);
  TORCH_CHECK(adc_bits == 0 || (adc_bits >= 2 && adc_bits <= 16), who,
              ": adc_bits must be 0 or 2..16, got ", adc_bits);
  TORCH_CHECK(sigma_mode != 0 || adc_bits != 0, who,
              ": noise (sigma_mode) and ADC (adc_bits) are both off");
  if (adc_bits > 0)
    TORCH_CHECK(adc.numel() == 2 && adc.scalar_type() == torch::kFloat32 &&
                    adc.is_contiguous() && adc.device() == x.device(),
                who, ": adc must be the fp32 device tensor [step, 1/step]");
}

// wq2 (and wr2, which may be wq2 again) are the [K, nrows] row matrices of x
inline void check_xbar_weights(const torch::Tensor& x, const ConvGeom& g,
                               const torch::Tensor& wq2,
                               const torch::Tensor& wr2, const char* who) {
  TORCH_CHECK(wq2.dim() == 2 && wq2.size(0) == g.K &&
                  wq2.size(1) == g.R * g.S * g.C && wr2.sizes() == wq2.sizes(),
              who, ": weight shape mismatch");
  TORCH_CHECK(wq2.scalar_type() == x.scalar_type() &&
                  wr2.scalar_type() == x.scalar_type(),
              who, ": x and the weights must share one dtype");
}

// row pitch of a [K, nrows] matrix as the kernels read it: the (small) rows
// of a 16-bit dtype are zero-padded to 8 elements so that the 16-byte row
// loads are aligned
inline int xbar_pitch(int nrows, size_t elem_size) {
  return elem_size == 2 ? (nrows + 7) & ~7 : nrows;
}

inline torch::Tensor pad_rows8(const torch::Tensor& w, int nrows,
                               size_t elem_size) {
  int pitch = xbar_pitch(nrows, elem_size);
  if (pitch == nrows) return w.contiguous();
  return at::constant_pad_nd(w, {0, pitch - nrows}, 0).contiguous();
}

// What every launch needs besides its weights: the fp32 bias, the telemetry
// and saturation buffers, the noise factor, the ADC pair, and the grid.
struct XbarLaunch {
  torch::Tensor bias_f, tele, sat, factor_f;
  const float* bias = nullptr;      // nullptr: no bias
  const float* factor = nullptr;
  const float* adc = nullptr;       // [step, 1/step]; nullptr: ADC off
  float* telem = nullptr;           // nullptr: telemetry off
  unsigned long long* sat_count = nullptr;
  bool adc_on;
  dim3 grid;

  XbarLaunch(const torch::Tensor& x, const torch::Tensor& bias_t,
             const ConvGeom& g, const torch::Tensor& factor_t,
             int64_t adc_bits, const torch::Tensor& adc_t, bool with_telem,
             const char* who)
      : adc_on(adc_bits > 0),
        grid((g.K + BN - 1) / BN, (int)((g.M + BM - 1) / BM)) {
    if (bias_t.numel() > 0) {
      TORCH_CHECK(bias_t.numel() == g.K, who, ": bias size mismatch");
      bias_f = bias_t.to(torch::kFloat32).contiguous();
      bias = bias_f.data_ptr<float>();
    }
    auto f32 = x.options().dtype(torch::kFloat32);
    if (with_telem) {
      tele = torch::zeros({5}, f32);
      tele[2] = -std::numeric_limits<float>::infinity();
      sat = torch::zeros({1}, x.options().dtype(torch::kLong));
      telem = tele.data_ptr<float>();
      sat_count = (unsigned long long*)sat.data_ptr<int64_t>();
    } else {
      tele = torch::empty({0}, f32);
    }
    factor_f = factor_t.to(torch::kFloat32).reshape({1}).contiguous();
    factor = factor_f.data_ptr<float>();
    if (adc_on) adc = adc_t.data_ptr<float>();
  }

  std::vector<torch::Tensor> finish(const torch::Tensor& out) {
    HIP_CHECK_LAST();
    if (telem) tele.narrow(0, 3, 1).copy_(sat);
    return {out, tele};
  }
};

// f(sigma_mode, adc, telem) with integral constants. check_xbar_args left
// exactly these modes: 0 (ADC on), 1, 2
template <typename F>
void xbar_dispatch_mode(int64_t sigma_mode, bool adc_on, bool telem, F&& f) {
  using TT = std::true_type; using FF = std::false_type;
  auto with_telem = [&](auto sm, auto ad) {
    if (telem) f(sm, ad, TT{}); else f(sm, ad, FF{});
  };
  auto with_adc = [&](auto sm) {
    if (adc_on) with_telem(sm, TT{}); else with_telem(sm, FF{});
  };
  if (sigma_mode == 0) with_telem(std::integral_constant<int, 0>{}, TT{});
  else if (sigma_mode == 1) with_adc(std::integral_constant<int, 1>{});
  else with_adc(std::integral_constant<int, 2>{});
}

// f(n) with the slice count (1..4, checked by the caller) as a constant
template <typename F>
void dispatch_slices(int n, F&& f) {
  if (n == 1) f(std::integral_constant<int, 1>{});
  else if (n == 2) f(std::integral_constant<int, 2>{});
  else if (n == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

// Geometry, output and weight-row view of a conv entry point. x, wq and (if
// given) wraw are channels_last; channels_last [K, C, R, S] is the raw
// [K, (r, s, c)] row matrix.
struct XbarConv {
  ConvGeom g;
  torch::Tensor out;

  XbarConv(const torch::Tensor& x, const torch::Tensor& wq,
           const torch::Tensor* wraw, int64_t stride, int64_t pad,
           const char* who) {
    const std::string name(who);
    check_cl(x, (name + " x").c_str());
    check_cl(wq, (name + " wq").c_str());
    if (wraw) check_cl(*wraw, (name + " wraw").c_str());
    TORCH_CHECK(wq.size(1) == x.size(1), who, ": channel mismatch");
    g = make_geom((int)x.size(0), (int)x.size(2), (int)x.size(3),
                  (int)x.size(1), (int)wq.size(0), (int)wq.size(2),
                  (int)wq.size(3), (int)stride, (int)pad);
    TORCH_CHECK(g.OH > 0 && g.OW > 0, who, ": empty output");
    out = torch::empty({g.N, g.K, g.OH, g.OW},
                       x.options().memory_format(at::MemoryFormat::ChannelsLast));
  }

  torch::Tensor rows(const torch::Tensor& w) const {
    return w.permute({0, 2, 3, 1}).reshape({(int64_t)g.K,
                                            (int64_t)g.R * g.S * g.C});
  }
};

}  // namespace
