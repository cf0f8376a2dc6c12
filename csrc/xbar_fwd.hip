// ===========================================================================
// Tiled crossbars: per-block current noise and ADC in one fused MFMA VMM.
//
// The contraction (crossbar rows) runs over the flat (r, s, c) filter order,
// c fastest -- for a linear layer the input index -- and is cut into blocks
// of xbar_rows rows (a positive multiple of the 32-row k-step; the last block
// may be short). Per block b and output (m, k):
//   p_b = sum x * wq                  s_b = max(sum x * f(|w_raw|), 0)
//   v_b = p_b + eps_b * sqrt(factor * s_b)       eps_b ~ N(0,1) per block
//   q_b = step * clamp(rint(v_b * inv_step), -Qm, Qm)
//   out = sum_b q_b + bias            (fp32, b ascending; rounded once)
// The block epilogue runs in registers on the live 2x2 accumulator fragments
// every xbar_rows/32 k-steps; no partial sum reaches memory. The Philox
// counter of a four-row group is (b*M + m)*K + k, so block 0 draws what the
// unblocked kernels draw and every block has counters of its own.
// Same 64x64 tile / 4 waves / BK = 32 structure as conv_fwd_kernel.
// ===========================================================================

#include "xbar_common.h"

namespace {

// SIGMA_MODE: 0 noise off, 1 abs, 2 abs2     ADC: quantise every block
// TELEM: telem[5] = sum sigma_abs, sum |sum_b noise_b|, max clean y,
//        (unused, see sat_count), max |v_b|; sat_count = number of block
//        partials with |rint(v_b / step)| > Qm (exact, 64-bit)
template <typename T, int SIGMA_MODE, bool ADC, bool TELEM, bool BIAS>
__global__ __launch_bounds__(kBlock)
void xbar_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                     const T* __restrict__ wraw,
                     const float* __restrict__ bias, T* __restrict__ out,
                     ConvGeom g, int wpitch, int xbar_rows,
                     const float* __restrict__ factor_p,
                     const float* __restrict__ adc_p /* step, 1/step */,
                     float qm, uint64_t seed, float* __restrict__ telem,
                     unsigned long long* __restrict__ sat_count,
                     const int64_t* __restrict__ seed_base) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  const float step = ADC ? adc_p[0] : 1.0f;
  const float inv_step = ADC ? adc_p[1] : 1.0f;
  int n0 = blockIdx.x * BN;
  int64_t m0 = (int64_t)blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                          // BM rows (x)
  char* b_lds = smem + BM * STR;               // BN rows (wq)
  char* c_lds = smem + (BM + BN) * STR;        // BN rows (f(|w_raw|))
  char* d_lds = smem + (BM + 2 * BN) * STR;    // BN rows (|w_raw|, telem)

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  XbarRow xr = xbar_row_init(g, m0);

  f32x4 acc[2][2] = {};     // p_b
  f32x4 sacc[2][2] = {};    // s_b
  f32x4 tacc[2][2] = {};    // sigma_abs of the block (telemetry, abs2)
  f32x4 oacc[2][2] = {};    // sum_b q_b
  f32x4 ycl[2][2] = {};     // sum_b p_b (telemetry)
  f32x4 ntot[2][2] = {};    // sum_b noise_b (telemetry)
  float t_sum_sigma = 0.0f, t_sat = 0.0f, t_vmax = 0.0f;

  const int nrows = g.R * g.S * g.C;
  const int steps_per_block = xbar_rows / BK;
  int steps_left = steps_per_block;
  int b = 0;
  XbarRegs<T> rg;
  xbar_load_x(rg.x, x, g, xr);
  xbar_load_w<T, SIGMA_MODE>(rg.q, rg.w, wq, wraw, g.K, n0, 0, nrows, wpitch);
  for (int ck = 0; ck < nrows; ck += BK) {
    {
      int row = threadIdx.x >> 2;
      int seg = threadIdx.x & 3;
      xbar_put8<T>(a_lds, row, seg, rg.x);
      xbar_store_w_tiles<T, SIGMA_MODE, TELEM>(b_lds, c_lds, d_lds, row, seg,
                                               rg);
    }
    __syncthreads();
    if (ck + BK < nrows) {  // next step's loads, in flight under the MFMAs
      xbar_row_advance(xr, g, BK);
      xbar_load_x(rg.x, x, g, xr);
      xbar_load_w<T, SIGMA_MODE>(rg.q, rg.w, wq, wraw, g.K, n0, ck + BK,
                                 nrows, wpitch);
    }
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      auto a = Mma<T>::load(a_lds, xbar_frag_row(wm, fm, lane), lane);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int brow = xbar_frag_row(wn, fn, lane);
        auto bq = Mma<T>::load(b_lds, brow, lane);
        Mma<T>::mma(a, bq, acc[fm][fn]);
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

    if (--steps_left > 0 && ck + BK < nrows) continue;
    // block boundary (or the end): noise + ADC on the live fragments
    steps_left = steps_per_block;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int64_t mb = xbar_frag_m(m0, wm, fm, lane);
        int n = xbar_frag_n(n0, wn, fn, lane);
        float g4[4] = {};
        if (SIGMA_MODE > 0)
          gauss4(seed, (uint64_t)(((int64_t)b * g.M + mb) * g.K + n), g4);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          bool inside = mb + reg < g.M && n < g.K;
          float p = acc[fm][fn][reg];
          float sig = (SIGMA_MODE > 0) ? fmaxf(sacc[fm][fn][reg], 0.0f) : 0.0f;
          XbarPartial c = xbar_convert<SIGMA_MODE, ADC, false>(
              p, sig, g4[reg], factor, step, inv_step, qm);
          if (TELEM) {
            if (SIGMA_MODE > 0) {
              ntot[fm][fn][reg] += c.noise;
              if (inside)
                t_sum_sigma += (SIGMA_MODE == 2) ? tacc[fm][fn][reg]
                                                 : sacc[fm][fn][reg];
            }
            if (ADC && inside && fabsf(c.t) > qm) t_sat += 1.0f;
            ycl[fm][fn][reg] += p;
            if (inside) t_vmax = fmaxf(t_vmax, fabsf(c.v));
          }
          oacc[fm][fn][reg] += c.q;
        }
        acc[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        sacc[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        tacc[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    ++b;
  }

  xbar_finish<T, SIGMA_MODE, ADC, TELEM, BIAS>(
      oacc, ycl, ntot, BIAS ? bias : nullptr, out, g, m0, n0, wid, wm, wn,
      lane, t_sum_sigma, t_sat, t_vmax, telem, sat_count);
}

// ---------------------------------------------------------------------------
// Differential columns: the positive and the negative part of the weights sit
// on two columns, each with its own non-negative current, its own noise draw
// and its own UNIPOLAR ADC; the two codes are subtracted digitally.
//   wq+ = max(wq, 0)   wq- = max(-wq, 0)     f+- = f(|w_raw|) by sign(w_raw)
//   p+- = sum x * wq+-                       s+- = max(sum x * f+-, 0)
//   v+- = p+- + eps+- * sqrt(factor * s+-)
//   q+- = step * clamp(rint(v+- * inv_step), 0, Qu)
//   out = sum_b (q+ - q-) + bias
// The split happens once per staged element, from the one wq and the one
// w_raw load, into four weight tiles (wq+, wq-, f+, f-): LDS is (64 + 4*64)
// rows, + 64 for |w_raw| (telemetry with abs2). Splitting the loaded
// fragments in registers instead would repeat the work in every wave and for
// every k-step fragment, and gfx950 has no packed bf16 max. The positive
// column of block b keeps the counter (b*M + m)*K + k, the negative column
// uses ((nblocks + b)*M + m)*K + k: with weights >= 0 and the ADC off this
// kernel draws and returns what xbar_fwd_kernel returns. Bias is a run-time
// branch here (bias == nullptr) to halve the instantiation count.
// ---------------------------------------------------------------------------

template <typename T, int SIGMA_MODE, bool TELEM>
DEV_INLINE void xbar_diff_store_tiles(char* a_lds, char* bp_lds, char* bn_lds,
                                      char* cp_lds, char* cn_lds, char* d_lds,
                                      const XbarRegs<T>& rg) {
  int row = threadIdx.x >> 2;
  int seg = threadIdx.x & 3;
  xbar_put8<T>(a_lds, row, seg, rg.x);
  float p[8], n[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float q = to_f32(rg.q[j]);
    p[j] = fmaxf(q, 0.0f);
    n[j] = fmaxf(-q, 0.0f);
  }
  Mma<T>::store8(bp_lds, row, seg * 8, p);
  Mma<T>::store8(bn_lds, row, seg * 8, n);
  if (SIGMA_MODE > 0) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float w = to_f32(rg.w[j]);
      a[j] = fabsf(w);
      float v = (SIGMA_MODE == 2) ? a[j] * a[j] + a[j] : a[j];
      p[j] = (w > 0.0f) ? v : 0.0f;
      n[j] = (w < 0.0f) ? v : 0.0f;
    }
    Mma<T>::store8(cp_lds, row, seg * 8, p);
    Mma<T>::store8(cn_lds, row, seg * 8, n);
    if (TELEM && SIGMA_MODE == 2) Mma<T>::store8(d_lds, row, seg * 8, a);
  }
}

// TELEM as in xbar_fwd_kernel, per column: telem[1] sums
// |sum_b (noise+ - noise-)|, sat_count counts column partials with
// rint(v / step) > Qu or < 0, telem[4] is the max |v+-|; qu = 2^bits - 1
template <typename T, int SIGMA_MODE, bool ADC, bool TELEM>
__global__ __launch_bounds__(kBlock)
void xbar_diff_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                          const T* __restrict__ wraw,
                          const float* __restrict__ bias, T* __restrict__ out,
                          ConvGeom g, int wpitch, int xbar_rows,
                          const float* __restrict__ factor_p,
                          const float* __restrict__ adc_p /* step, 1/step */,
                          float qu, uint64_t seed, float* __restrict__ telem,
                          unsigned long long* __restrict__ sat_count,
                          const int64_t* __restrict__ seed_base) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  const float step = ADC ? adc_p[0] : 1.0f;
  const float inv_step = ADC ? adc_p[1] : 1.0f;
  int n0 = blockIdx.x * BN;
  int64_t m0 = (int64_t)blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                          // BM rows (x)
  char* bp_lds = smem + BM * STR;              // BN rows (wq+)
  char* bn_lds = smem + (BM + BN) * STR;       // BN rows (wq-)
  char* cp_lds = smem + (BM + 2 * BN) * STR;   // BN rows (f+)
  char* cn_lds = smem + (BM + 3 * BN) * STR;   // BN rows (f-)
  char* d_lds = smem + (BM + 4 * BN) * STR;    // BN rows (|w_raw|, telem)

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  XbarRow xr = xbar_row_init(g, m0);

  f32x4 accp[2][2] = {}, accn[2][2] = {};     // p+, p-
  f32x4 saccp[2][2] = {}, saccn[2][2] = {};   // s+, s-
  f32x4 tacc[2][2] = {};    // sigma_abs of the block (telemetry, abs2)
  f32x4 oacc[2][2] = {};    // sum_b (q+ - q-)
  f32x4 ycl[2][2] = {};     // sum_b (p+ - p-) (telemetry)
  f32x4 ntot[2][2] = {};    // sum_b (noise+ - noise-) (telemetry)
  float t_sum_sigma = 0.0f, t_sat = 0.0f, t_vmax = 0.0f;

  const int nrows = g.R * g.S * g.C;
  const int nblocks = (nrows + xbar_rows - 1) / xbar_rows;
  const int steps_per_block = xbar_rows / BK;
  int steps_left = steps_per_block;
  int b = 0;
  XbarRegs<T> rg;
  xbar_load_x(rg.x, x, g, xr);
  xbar_load_w<T, SIGMA_MODE>(rg.q, rg.w, wq, wraw, g.K, n0, 0, nrows, wpitch);
  for (int ck = 0; ck < nrows; ck += BK) {
    xbar_diff_store_tiles<T, SIGMA_MODE, TELEM>(a_lds, bp_lds, bn_lds, cp_lds,
                                                cn_lds, d_lds, rg);
    __syncthreads();
    if (ck + BK < nrows) {  // next step's loads, in flight under the MFMAs
      xbar_row_advance(xr, g, BK);
      xbar_load_x(rg.x, x, g, xr);
      xbar_load_w<T, SIGMA_MODE>(rg.q, rg.w, wq, wraw, g.K, n0, ck + BK,
                                 nrows, wpitch);
    }
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      auto a = Mma<T>::load(a_lds, xbar_frag_row(wm, fm, lane), lane);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int brow = xbar_frag_row(wn, fn, lane);
        auto bqp = Mma<T>::load(bp_lds, brow, lane);
        Mma<T>::mma(a, bqp, accp[fm][fn]);
        auto bqn = Mma<T>::load(bn_lds, brow, lane);
        Mma<T>::mma(a, bqn, accn[fm][fn]);
        if (SIGMA_MODE > 0) {
          auto bsp = Mma<T>::load(cp_lds, brow, lane);
          Mma<T>::mma(a, bsp, saccp[fm][fn]);
          auto bsn = Mma<T>::load(cn_lds, brow, lane);
          Mma<T>::mma(a, bsn, saccn[fm][fn]);
        }
        if (TELEM && SIGMA_MODE == 2) {
          auto bt = Mma<T>::load(d_lds, brow, lane);
          Mma<T>::mma(a, bt, tacc[fm][fn]);
        }
      }
    }
    __syncthreads();

    if (--steps_left > 0 && ck + BK < nrows) continue;
    // block boundary (or the end): noise + ADC on both columns' fragments
    steps_left = steps_per_block;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int64_t mb = xbar_frag_m(m0, wm, fm, lane);
        int n = xbar_frag_n(n0, wn, fn, lane);
        float gp[4] = {}, gn[4] = {};
        if (SIGMA_MODE > 0) {
          gauss4(seed, (uint64_t)(((int64_t)b * g.M + mb) * g.K + n), gp);
          gauss4(seed,
                 (uint64_t)(((int64_t)(nblocks + b) * g.M + mb) * g.K + n), gn);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          bool inside = mb + reg < g.M && n < g.K;
          float pp = accp[fm][fn][reg], pn = accn[fm][fn][reg];
          // The two columns stay interleaved stage by stage, written out
          // here: sent one after the other through xbar_convert, the ADC +
          // telemetry instantiations contracted other multiply-adds and 33
          // of 3,294 fingerprint cases changed in the last bit.
          float vp = pp, vn = pn;
          if (SIGMA_MODE > 0) {
            float sp = fmaxf(saccp[fm][fn][reg], 0.0f);
            float sn = fmaxf(saccn[fm][fn][reg], 0.0f);
            float noisep = gp[reg] * sqrtf(factor * sp);
            float noisen = gn[reg] * sqrtf(factor * sn);
            vp = pp + noisep;
            vn = pn + noisen;
            if (TELEM) {
              ntot[fm][fn][reg] += noisep - noisen;
              if (inside)
                t_sum_sigma += (SIGMA_MODE == 2)
                                   ? tacc[fm][fn][reg]
                                   : saccp[fm][fn][reg] + saccn[fm][fn][reg];
            }
          }
          float qp = vp, qn = vn;
          if (ADC) {
            float tp = rintf(vp * inv_step);
            float tn = rintf(vn * inv_step);
            if (TELEM && inside) {
              if (tp > qu || tp < 0.0f) t_sat += 1.0f;
              if (tn > qu || tn < 0.0f) t_sat += 1.0f;
            }
            qp = step * fminf(fmaxf(tp, 0.0f), qu);
            qn = step * fminf(fmaxf(tn, 0.0f), qu);
          }
          if (TELEM) {
            ycl[fm][fn][reg] += pp - pn;
            if (inside)
              t_vmax = fmaxf(t_vmax, fmaxf(fabsf(vp), fabsf(vn)));
          }
          oacc[fm][fn][reg] += qp - qn;
        }
        accp[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        accn[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        saccp[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        saccn[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        tacc[fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    ++b;
  }

  xbar_finish<T, SIGMA_MODE, ADC, TELEM>(oacc, ycl, ntot, bias, out, g, m0, n0,
                                         wid, wm, wn, lane, t_sum_sigma, t_sat,
                                         t_vmax, telem, sat_count);
}

// x, wq2, wr2 are raw NHWC / [K, nrows] row-matrix views; out is allocated by
// the caller with M*K elements in [M, K] raw order
std::vector<torch::Tensor> xbar_fwd_impl(
    const torch::Tensor& x, torch::Tensor wq2, torch::Tensor wr2,
    const torch::Tensor& bias, ConvGeom g, torch::Tensor out,
    int64_t sigma_mode, const torch::Tensor& factor, int64_t xbar_rows,
    int64_t adc_bits, const torch::Tensor& adc, int64_t seed, bool telem,
    bool diff, const char* who) {
  check_xbar_args(sigma_mode, xbar_rows, adc_bits, adc, x, who);
  check_xbar_weights(x, g, wq2, wr2, who);
  const int nrows = g.R * g.S * g.C;
  const int pitch = xbar_pitch(nrows, x.element_size());
  const bool same = wr2.is_same(wq2);
  wq2 = pad_rows8(wq2, nrows, x.element_size());
  wr2 = same ? wq2 : pad_rows8(wr2, nrows, x.element_size());
  XbarLaunch L(x, bias, g, factor, adc_bits, adc, telem, who);
  // top ADC code: bipolar +-Qm, or unipolar 0..Qu on differential columns
  float qm = !L.adc_on ? 0.0f
             : diff    ? (float)((1 << adc_bits) - 1)
                       : (float)((1 << (adc_bits - 1)) - 1);
  NN_DISPATCH(x.scalar_type(), "xbar_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    size_t lds = (size_t)(BM + (diff ? 5 : 3) * BN) * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq2.data_ptr();
    const T* wrp = (const T*)wr2.data_ptr();
    T* op = (T*)out.data_ptr();
    uint64_t sd = (uint64_t)seed;
    using TT = std::true_type; using FF = std::false_type;
    xbar_dispatch_mode(sigma_mode, L.adc_on, telem,
                       [&](auto sm, auto ad, auto tl) {
      auto launch = [&](auto bi) {
        hipLaunchKernelGGL((xbar_fwd_kernel<T, decltype(sm)::value,
                            decltype(ad)::value, decltype(tl)::value,
                            decltype(bi)::value>), L.grid, dim3(kBlock), lds,
                           stream, xp, wqp, wrp, L.bias, op, g, pitch,
                           (int)xbar_rows, L.factor, L.adc, qm, sd, L.telem,
                           L.sat_count, g_seed_base);
      };
      if (diff)
        hipLaunchKernelGGL((xbar_diff_fwd_kernel<T, decltype(sm)::value,
                            decltype(ad)::value, decltype(tl)::value>),
                           L.grid, dim3(kBlock), lds, stream, xp, wqp, wrp,
                           L.bias, op, g, pitch, (int)xbar_rows, L.factor,
                           L.adc, qm, sd, L.telem, L.sat_count, g_seed_base);
      else if (L.bias) launch(TT{});
      else launch(FF{});
    });
  });
  return L.finish(out);
}

std::vector<torch::Tensor> xbar_conv_entry(
    const torch::Tensor& x, const torch::Tensor& wq, const torch::Tensor& wraw,
    const torch::Tensor& bias, int64_t stride, int64_t pad, int64_t sigma_mode,
    const torch::Tensor& factor, int64_t xbar_rows, int64_t adc_bits,
    const torch::Tensor& adc, int64_t seed, bool telem, bool diff,
    const char* who) {
  XbarConv cv(x, wq, &wraw, stride, pad, who);
  auto wq2 = cv.rows(wq);
  auto wr2 = wraw.is_same(wq) ? wq2 : cv.rows(wraw);
  return xbar_fwd_impl(x, wq2, wr2, bias, cv.g, cv.out, sigma_mode, factor,
                       xbar_rows, adc_bits, adc, seed, telem, diff, who);
}

std::vector<torch::Tensor> xbar_linear_entry(
    const torch::Tensor& x, const torch::Tensor& wq, const torch::Tensor& wraw,
    const torch::Tensor& bias, int64_t sigma_mode, const torch::Tensor& factor,
    int64_t xbar_rows, int64_t adc_bits, const torch::Tensor& adc,
    int64_t seed, bool telem, bool diff, const char* who) {
  TORCH_CHECK(wq.dim() == 2 && wq.size(1) == x.size(1), who,
              ": weight shape mismatch");
  auto g = linear_geom(x, wq.size(0));
  auto out = torch::empty({x.size(0), wq.size(0)}, x.options());
  return xbar_fwd_impl(x, wq, wraw, bias, g, out, sigma_mode, factor,
                       xbar_rows, adc_bits, adc, seed, telem, diff, who);
}

}  // namespace

std::vector<torch::Tensor> xbar_fwd_conv(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t xbar_rows, int64_t adc_bits, torch::Tensor adc, int64_t seed,
    bool telem) {
  return xbar_conv_entry(x, wq, wraw, bias, stride, pad, sigma_mode, factor,
                         xbar_rows, adc_bits, adc, seed, telem, false,
                         "xbar_fwd_conv");
}

std::vector<torch::Tensor> xbar_fwd_linear(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t sigma_mode, torch::Tensor factor, int64_t xbar_rows,
    int64_t adc_bits, torch::Tensor adc, int64_t seed, bool telem) {
  return xbar_linear_entry(x, wq, wraw, bias, sigma_mode, factor, xbar_rows,
                           adc_bits, adc, seed, telem, false,
                           "xbar_fwd_linear");
}

// differential columns (W+ / W- with unipolar per-column ADCs): same
// arguments; adc is [step, 1/step] of the unipolar step adc_max / (2^bits - 1)
std::vector<torch::Tensor> xbar_diff_fwd_conv(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t xbar_rows, int64_t adc_bits, torch::Tensor adc, int64_t seed,
    bool telem) {
  return xbar_conv_entry(x, wq, wraw, bias, stride, pad, sigma_mode, factor,
                         xbar_rows, adc_bits, adc, seed, telem, true,
                         "xbar_diff_fwd_conv");
}

std::vector<torch::Tensor> xbar_diff_fwd_linear(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t sigma_mode, torch::Tensor factor, int64_t xbar_rows,
    int64_t adc_bits, torch::Tensor adc, int64_t seed, bool telem) {
  return xbar_linear_entry(x, wq, wraw, bias, sigma_mode, factor, xbar_rows,
                           adc_bits, adc, seed, telem, true,
                           "xbar_diff_fwd_linear");
}
