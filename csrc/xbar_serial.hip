// ---------------------------------------------------------------------------
// Bit-serial inputs: the activation is a B-bit code on the grid x_step and
// reaches the rows D bits per cycle, J = ceil(B / D) cycles ("slices"). Every
// slice of every block has its own column current, noise draw and ADC
// conversion; the digital side shift-adds the slices.
//   code = clamp(rint(f32(x) * inv_x_step), 0, 2^B - 1)
//   d_j  = (code >> j*D) & (2^D - 1)                       j = 0..J-1
//   p_bj = x_step * sum d_j * wq    s_bj = max(x_step * sum d_j * f(|w_raw|), 0)
//   v_bj = p_bj + eps_bj * sqrt(factor * s_bj)
//   q_bj = step * clamp(rint(v_bj * inv_step), -Qm, Qm)
//   out  = sum_b sum_j 2^(jD) * q_bj + bias      (b ascending, j inside b)
// The MFMA operands are the integers d_j (exact in every dtype); x_step
// multiplies the fp32 accumulators in the epilogue. The staging thread derives
// the code once from its 8 activations and writes J activation tiles; the wq
// and f(|w_raw|) tiles are staged once per k-step and serve every slice, so a
// k-step costs J x the MFMAs of xbar_fwd_kernel but the same global loads and
// weight staging. Each slice has p and s accumulator fragments of its own; J
// is a template parameter so that they stay in registers. The Philox counter
// of a four-row group is ((b*J + j)*M + m)*K + k: with J = 1 this kernel
// draws what xbar_fwd_kernel draws. Bias is a run-time branch.
// ---------------------------------------------------------------------------

#include "xbar_common.h"

namespace {

// TELEM: telem[5] = sum_bj 2^(jD) sigma_abs_bj, sum |sum_bj 2^(jD) noise_bj|,
//        max clean shift-added y, (unused, see sat_count), max |v_bj|;
//        sat_count = number of (b, j) partials with |rint(v_bj / step)| > Qm
template <typename T, int J, int SIGMA_MODE, bool ADC, bool TELEM>
__global__ __launch_bounds__(kBlock)
void xbar_serial_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                            const T* __restrict__ wraw,
                            const float* __restrict__ bias,
                            T* __restrict__ out, ConvGeom g, int wpitch,
                            int xbar_rows, int in_bits, int dac_bits,
                            const float* __restrict__ dac_p /* x_step, 1/x_step */,
                            const float* __restrict__ factor_p,
                            const float* __restrict__ adc_p /* step, 1/step */,
                            float qm, uint64_t seed, float* __restrict__ telem,
                            unsigned long long* __restrict__ sat_count,
                            const int64_t* __restrict__ seed_base) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  const float step = ADC ? adc_p[0] : 1.0f;
  const float inv_step = ADC ? adc_p[1] : 1.0f;
  const float x_step = dac_p[0];
  const float inv_x_step = dac_p[1];
  const float code_max = (float)((1 << in_bits) - 1);
  const int dmask = (1 << dac_bits) - 1;
  int n0 = blockIdx.x * BN;
  int64_t m0 = (int64_t)blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                              // J x BM rows (d_j)
  char* b_lds = smem + J * BM * STR;               // BN rows (wq)
  char* c_lds = smem + (J * BM + BN) * STR;        // BN rows (f(|w_raw|))
  char* d_lds = smem + (J * BM + 2 * BN) * STR;    // BN rows (|w_raw|, telem)

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  XbarRow xr = xbar_row_init(g, m0);

  f32x4 acc[J][2][2] = {};    // sum d_j * wq of the block
  f32x4 sacc[J][2][2] = {};   // sum d_j * f(|w_raw|) of the block
  f32x4 tacc[J][2][2] = {};   // sum d_j * |w_raw| (telemetry, abs2)
  f32x4 oacc[2][2] = {};      // sum_bj 2^(jD) q_bj
  f32x4 ycl[2][2] = {};       // sum_bj 2^(jD) p_bj (telemetry)
  f32x4 ntot[2][2] = {};      // sum_bj 2^(jD) noise_bj (telemetry)
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
      // the code, once; then one activation tile per slice
      int row = threadIdx.x >> 2;
      int seg = threadIdx.x & 3;
      int code[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        code[e] = xbar_code(to_f32(rg.x[e]), 0.0f, inv_x_step, code_max);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        float d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          d[e] = xbar_digit(code[e], j, dac_bits, dmask);
        Mma<T>::store8(a_lds + j * BM * STR, row, seg * 8, d);
      }
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
      typename Mma<T>::frag a[J];
#pragma unroll
      for (int j = 0; j < J; ++j)
        a[j] = Mma<T>::load(a_lds + j * BM * STR, xbar_frag_row(wm, fm, lane),
                            lane);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int brow = xbar_frag_row(wn, fn, lane);
        auto bq = Mma<T>::load(b_lds, brow, lane);
#pragma unroll
        for (int j = 0; j < J; ++j) Mma<T>::mma(a[j], bq, acc[j][fm][fn]);
        if (SIGMA_MODE > 0) {
          auto bs = Mma<T>::load(c_lds, brow, lane);
#pragma unroll
          for (int j = 0; j < J; ++j) Mma<T>::mma(a[j], bs, sacc[j][fm][fn]);
        }
        if (TELEM && SIGMA_MODE == 2) {
          auto bt = Mma<T>::load(d_lds, brow, lane);
#pragma unroll
          for (int j = 0; j < J; ++j) Mma<T>::mma(a[j], bt, tacc[j][fm][fn]);
        }
      }
    }
    __syncthreads();

    if (--steps_left > 0 && ck + BK < nrows) continue;
    // block boundary (or the end): J noise draws and J ADCs on the live
    // fragments, shift-added into the output
    steps_left = steps_per_block;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int64_t mb = xbar_frag_m(m0, wm, fm, lane);
        int n = xbar_frag_n(n0, wn, fn, lane);
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const float shift = (float)(1 << (j * dac_bits));
          float g4[4] = {};
          if (SIGMA_MODE > 0)
            gauss4(seed,
                   (uint64_t)((((int64_t)b * J + j) * g.M + mb) * g.K + n),
                   g4);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            bool inside = mb + reg < g.M && n < g.K;
            float p = __fmul_rn(x_step, acc[j][fm][fn][reg]);
            float sig = (SIGMA_MODE > 0)
                ? fmaxf(__fmul_rn(x_step, sacc[j][fm][fn][reg]), 0.0f) : 0.0f;
            XbarPartial c = xbar_convert<SIGMA_MODE, ADC, false>(
                p, sig, g4[reg], factor, step, inv_step, qm);
            if (TELEM) {
              if (SIGMA_MODE > 0) {
                ntot[fm][fn][reg] += shift * c.noise;
                if (inside)
                  t_sum_sigma += shift * x_step
                      * ((SIGMA_MODE == 2) ? tacc[j][fm][fn][reg]
                                           : sacc[j][fm][fn][reg]);
              }
              if (ADC && inside && fabsf(c.t) > qm) t_sat += 1.0f;
              ycl[fm][fn][reg] += shift * p;
              if (inside) t_vmax = fmaxf(t_vmax, fabsf(c.v));
            }
            oacc[fm][fn][reg] += shift * c.q;
          }
          acc[j][fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          sacc[j][fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          tacc[j][fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
      }
    }
    ++b;
  }

  xbar_finish<T, SIGMA_MODE, ADC, TELEM>(oacc, ycl, ntot, bias, out, g, m0, n0,
                                         wid, wm, wn, lane, t_sum_sigma, t_sat,
                                         t_vmax, telem, sat_count);
}

// slice count of a bit-serial call, after checking in_bits / dac_bits / dac
int check_xbar_serial_args(int64_t in_bits, int64_t dac_bits,
                           const torch::Tensor& dac, const torch::Tensor& x,
                           const char* who) {
  int64_t top = x.scalar_type() == torch::kBFloat16 ? 7 : 8;
  TORCH_CHECK(in_bits >= 1 && in_bits <= top, who, ": in_bits must be 1..",
              top, " for ", x.scalar_type(), " activations (bf16 does not "
              "carry every 8-bit code), got ", in_bits);
  TORCH_CHECK(dac_bits >= 1, who, ": dac_bits must be >= 1, got ", dac_bits);
  int64_t J = (in_bits + dac_bits - 1) / dac_bits;
  TORCH_CHECK(J <= 4, who, ": in_bits ", in_bits, " at dac_bits ", dac_bits,
              " is ", J, " slices, at most 4 are built; the smallest "
              "dac_bits that works is ", (in_bits + 3) / 4);
  TORCH_CHECK(dac.numel() == 2 && dac.scalar_type() == torch::kFloat32 &&
                  dac.is_contiguous() && dac.device() == x.device(),
              who, ": dac must be the fp32 device tensor [x_step, 1/x_step]");
  return (int)J;
}

// x, wq2, wr2 are raw NHWC / [K, nrows] row-matrix views; out is allocated by
// the caller with M*K elements in [M, K] raw order
std::vector<torch::Tensor> xbar_serial_fwd_impl(
    const torch::Tensor& x, torch::Tensor wq2, torch::Tensor wr2,
    const torch::Tensor& bias, ConvGeom g, torch::Tensor out,
    int64_t sigma_mode, const torch::Tensor& factor, int64_t xbar_rows,
    int64_t adc_bits, const torch::Tensor& adc, int64_t in_bits,
    int64_t dac_bits, const torch::Tensor& dac, int64_t seed, bool telem,
    const char* who) {
  check_xbar_args(sigma_mode, xbar_rows, adc_bits, adc, x, who);
  const int J = check_xbar_serial_args(in_bits, dac_bits, dac, x, who);
  check_xbar_weights(x, g, wq2, wr2, who);
  const int nrows = g.R * g.S * g.C;
  const int pitch = xbar_pitch(nrows, x.element_size());
  const bool same = wr2.is_same(wq2);
  wq2 = pad_rows8(wq2, nrows, x.element_size());
  wr2 = same ? wq2 : pad_rows8(wr2, nrows, x.element_size());
  XbarLaunch L(x, bias, g, factor, adc_bits, adc, telem, who);
  float qm = L.adc_on ? (float)((1 << (adc_bits - 1)) - 1) : 0.0f;
  NN_DISPATCH(x.scalar_type(), "xbar_serial_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    // at most (4 * 64 + 3 * 64) * 144 = 64512 bytes (fp32, four slices)
    size_t lds = (size_t)(J * BM + 3 * BN) * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq2.data_ptr();
    const T* wrp = (const T*)wr2.data_ptr();
    T* op = (T*)out.data_ptr();
    const float* dp = dac.data_ptr<float>();
    uint64_t sd = (uint64_t)seed;
    dispatch_slices(J, [&](auto jj) {
      xbar_dispatch_mode(sigma_mode, L.adc_on, telem,
                         [&](auto sm, auto ad, auto tl) {
        hipLaunchKernelGGL((xbar_serial_fwd_kernel<T, decltype(jj)::value,
                            decltype(sm)::value, decltype(ad)::value,
                            decltype(tl)::value>), L.grid, dim3(kBlock), lds,
                           stream, xp, wqp, wrp, L.bias, op, g, pitch,
                           (int)xbar_rows, (int)in_bits, (int)dac_bits, dp,
                           L.factor, L.adc, qm, sd, L.telem, L.sat_count,
                           g_seed_base);
      });
    });
  });
  return L.finish(out);
}

}  // namespace

// bit-serial inputs (in_bits-bit codes on the grid x_step, dac_bits per
// slice); dac = fp32 [x_step, 1/x_step]
std::vector<torch::Tensor> xbar_serial_fwd_conv(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t xbar_rows, int64_t adc_bits, torch::Tensor adc, int64_t in_bits,
    int64_t dac_bits, torch::Tensor dac, int64_t seed, bool telem) {
  const char* who = "xbar_serial_fwd_conv";
  XbarConv cv(x, wq, &wraw, stride, pad, who);
  auto wq2 = cv.rows(wq);
  auto wr2 = wraw.is_same(wq) ? wq2 : cv.rows(wraw);
  return xbar_serial_fwd_impl(x, wq2, wr2, bias, cv.g, cv.out, sigma_mode,
                              factor, xbar_rows, adc_bits, adc, in_bits,
                              dac_bits, dac, seed, telem, who);
}

std::vector<torch::Tensor> xbar_serial_fwd_linear(
    torch::Tensor x, torch::Tensor wq, torch::Tensor wraw, torch::Tensor bias,
    int64_t sigma_mode, torch::Tensor factor, int64_t xbar_rows,
    int64_t adc_bits, torch::Tensor adc, int64_t in_bits, int64_t dac_bits,
    torch::Tensor dac, int64_t seed, bool telem) {
  const char* who = "xbar_serial_fwd_linear";
  TORCH_CHECK(wq.dim() == 2 && wq.size(1) == x.size(1), who,
              ": weight shape mismatch");
  auto g = linear_geom(x, wq.size(0));
  auto out = torch::empty({x.size(0), wq.size(0)}, x.options());
  return xbar_serial_fwd_impl(x, wq, wraw, bias, g, out, sigma_mode, factor,
                              xbar_rows, adc_bits, adc, in_bits, dac_bits,
                              dac, seed, telem, who);
}
