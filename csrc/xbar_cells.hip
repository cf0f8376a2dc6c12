// ---------------------------------------------------------------------------
// Bit-sliced weights: a cell holds E bits, so the B-bit weight code (offset
// binary on the weight quantiser's grid w = w_min + code * w_step) is spread
// over NSLICE = ceil(B / E) columns. Every column of every block has its own
// current, noise draw and UNIPOLAR ADC conversion; the digital side shift-adds
// the columns and adds the offset w_min * sum x.
//   code = clamp(rint((f32(wq) - w_min) * inv_w_step), 0, 2^B - 1)
//   d_t  = (code >> t*E) & (2^E - 1)                       t = 0..NSLICE-1
//   p_bt = w_step * sum x * d_t
//   s_bt = max(p_bt, 0)                                    (abs: g = w_step d)
//        = max(w_step^2 * sum x * d_t^2 + p_bt, 0)         (abs2: g^2 + g)
//   v_bt = p_bt + eps_bt * sqrt(factor * s_bt)
//   q_bt = step * clamp(rint(v_bt * inv_step), 0, Qu)
//   X_b  = sum x
//   out  = sum_b (sum_t 2^(tE) q_bt + w_min * X_b) + bias
// (b ascending, t ascending inside b, the offset after the block's columns).
// The MFMA operands are the activation and the integers d_t, d_t^2 <= 225
// (exact in every dtype); w_step and w_step^2 multiply the fp32 accumulators
// in the epilogue, so abs mode needs no sigma MFMA at all; neither does abs2
// with one-bit cells, where d_t^2 = d_t: the host then launches the abs
// instantiation with ``fold_squares`` set and the epilogue adds
// w_step^2 * sum x * d_t from the one accumulator. The staging thread
// derives the code once from its 8 wq elements and writes NSLICE digit tiles
// (and NSLICE tiles of d_t^2 with abs2); the activation tile is staged once
// per k-step and serves every column. X_b is one MFMA per fm against an
// all-ones B fragment held in registers: every column of the result is the
// row sum, so it serves both fn. w_raw is not read: the conductances are the
// digits. The Philox counter of a four-row group is
// ((b*NSLICE + t)*M + m)*K + k: with one slice, w_step 1 and w_min 0 this
// kernel draws what xbar_fwd_kernel draws. Bias is a run-time branch.
// ---------------------------------------------------------------------------

#include "xbar_common.h"

namespace {

// TELEM: telem[5] = sum_bt p_bt (the current the cells draw, NOT
//        shift-weighted), sum |sum_bt 2^(tE) noise_bt|, max clean shift-added
//        y with the offset and the bias, (unused, see sat_count), max |v_bt|;
//        sat_count = number of (b, t) partials with rint(v_bt / step) > Qu
//        or < 0
//
// PROG ("programmed cells"): the conductances are DATA, not digits. ``cells``
// is G[NSLICE][K][wpitch] in digit units, written once per layer by
// xbar_program_cells_kernel (device-to-device variation, stuck-at cells):
//   p_bt = w_step * sum x * G_t
//   s_bt = max(p_bt, 0)                                                (abs)
//        = max(w_step^2 * sum x * round_to_dtype(f32(G_t)^2) + p_bt, 0) (abs2)
// and everything from v_bt on is the model above. The staging thread loads
// its 8-span of each of the NSLICE slices of G (in flight under the MFMAs,
// as the wq span is), stores them as the conductance tiles and, with abs2,
// their squares (fp32, rounded once). wq is not read; spans past K or past
// the contraction are zeros. G^2 != G, so ``fold_squares`` is never set.
template <typename T, int NSLICE, int SIGMA_MODE, bool ADC, bool TELEM,
          bool PROG>
__global__ __launch_bounds__(kBlock)
void xbar_cells_fwd_kernel(const T* __restrict__ x, const T* __restrict__ wq,
                           const float* __restrict__ bias,
                           T* __restrict__ out, ConvGeom g, int wpitch,
                           int xbar_rows, int w_bits, int cell_bits,
                           int fold_squares /* abs2 on one-bit cells */,
                           const float* __restrict__ cell_p /* w_step, 1/w_step, w_min */,
                           const float* __restrict__ factor_p,
                           const float* __restrict__ adc_p /* step, 1/step */,
                           float qu, uint64_t seed, float* __restrict__ telem,
                           unsigned long long* __restrict__ sat_count,
                           const int64_t* __restrict__ seed_base,
                           const T* __restrict__ cells /* PROG: G */,
                           int64_t cell_stride /* K * wpitch */) {
  seed = graph_seed(seed_base, seed);
  const float factor = (SIGMA_MODE > 0) ? factor_p[0] : 0.0f;
  const float step = ADC ? adc_p[0] : 1.0f;
  const float inv_step = ADC ? adc_p[1] : 1.0f;
  const float w_step = cell_p[0];
  const float inv_w_step = cell_p[1];
  const float w_min = cell_p[2];
  const float w_step2 = __fmul_rn(w_step, w_step);
  // SIGMA_MODE 1: s = sq1 * sum x * d_t + p_bt with sq1 = 0 (abs, s = p_bt
  // exactly) or w_step^2 (abs2 on one-bit cells)
  const float sq1 = fold_squares ? w_step2 : 0.0f;
  const float code_max = (float)((1 << w_bits) - 1);
  const int dmask = (1 << cell_bits) - 1;
  int n0 = blockIdx.x * BN;
  int64_t m0 = (int64_t)blockIdx.y * BM;

  constexpr int STR = Mma<T>::STRIDE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                               // BM rows (x)
  char* d_lds = smem + BM * STR;                    // NSLICE x BN rows (d_t)
  char* e_lds = smem + (BM + NSLICE * BN) * STR;    // NSLICE x BN rows (d_t^2)

  int wid = threadIdx.x / WAVE;
  int wm = wid >> 1, wn = wid & 1;
  int lane = threadIdx.x & (WAVE - 1);

  XbarRow xr = xbar_row_init(g, m0);

  typename Mma<T>::frag ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = 1.0f;

  f32x4 acc[NSLICE][2][2] = {};    // sum x * d_t of the block
  f32x4 sacc[NSLICE][2][2] = {};   // sum x * d_t^2 of the block (abs2)
  f32x4 xacc[2] = {};              // X_b = sum x of the block, per fm
  f32x4 oacc[2][2] = {};           // sum_b (sum_t 2^(tE) q_bt + w_min X_b)
  f32x4 ycl[2][2] = {};            // the same with p_bt for q_bt (telemetry)
  f32x4 ntot[2][2] = {};           // sum_bt 2^(tE) noise_bt (telemetry)
  float t_sum_sigma = 0.0f, t_sat = 0.0f, t_vmax = 0.0f;

  const int nrows = g.R * g.S * g.C;
  const int steps_per_block = xbar_rows / BK;
  int steps_left = steps_per_block;
  int b = 0;
  XbarRegs<T> rg;   // rg.w stays unused: the conductances are the digits
  // PROG: the thread's span of every slice of G, in place of rg.q
  alignas(16) T gq[PROG ? NSLICE : 1][8];
  xbar_load_x(rg.x, x, g, xr);
  if (PROG) {
#pragma unroll
    for (int t = 0; t < NSLICE; ++t)
      xbar_load_w<T, 0>(gq[PROG ? t : 0], rg.w, cells + t * cell_stride, cells,
                        g.K, n0, 0, nrows, wpitch);
  } else {
    xbar_load_w<T, 0>(rg.q, rg.w, wq, wq, g.K, n0, 0, nrows, wpitch);
  }
  for (int ck = 0; ck < nrows; ck += BK) {
    if (PROG) {
      // the conductance tiles as they are; squares in fp32, rounded once
      int row = threadIdx.x >> 2;
      int seg = threadIdx.x & 3;
      xbar_put8<T>(a_lds, row, seg, rg.x);
#pragma unroll
      for (int t = 0; t < NSLICE; ++t) {
        xbar_put8<T>(d_lds + t * BN * STR, row, seg, gq[PROG ? t : 0]);
        if (SIGMA_MODE == 2) {
          float d[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float gv = to_f32(gq[PROG ? t : 0][e]);
            d[e] = __fmul_rn(gv, gv);
          }
          Mma<T>::store8(e_lds + t * BN * STR, row, seg * 8, d);
        }
      }
    } else {
      // the code, once; then one digit tile (and one of squares) per slice.
      // Rows past the contraction or past K stage the code of a zero weight:
      // their activations are zero / their outputs are never stored
      int row = threadIdx.x >> 2;
      int seg = threadIdx.x & 3;
      xbar_put8<T>(a_lds, row, seg, rg.x);
      int code[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        code[e] = xbar_code(to_f32(rg.q[e]), w_min, inv_w_step, code_max);
#pragma unroll
      for (int t = 0; t < NSLICE; ++t) {
        float d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          d[e] = xbar_digit(code[e], t, cell_bits, dmask);
        Mma<T>::store8(d_lds + t * BN * STR, row, seg * 8, d);
        if (SIGMA_MODE == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] *= d[e];
          Mma<T>::store8(e_lds + t * BN * STR, row, seg * 8, d);
        }
      }
    }
    __syncthreads();
    if (ck + BK < nrows) {  // next step's loads, in flight under the MFMAs
      xbar_row_advance(xr, g, BK);
      xbar_load_x(rg.x, x, g, xr);
      if (PROG) {
#pragma unroll
        for (int t = 0; t < NSLICE; ++t)
          xbar_load_w<T, 0>(gq[PROG ? t : 0], rg.w, cells + t * cell_stride,
                            cells, g.K, n0, ck + BK, nrows, wpitch);
      } else {
        xbar_load_w<T, 0>(rg.q, rg.w, wq, wq, g.K, n0, ck + BK, nrows, wpitch);
      }
    }
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      auto a = Mma<T>::load(a_lds, xbar_frag_row(wm, fm, lane), lane);
      Mma<T>::mma(a, ones, xacc[fm]);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int brow = xbar_frag_row(wn, fn, lane);
#pragma unroll
        for (int t = 0; t < NSLICE; ++t) {
          auto bd = Mma<T>::load(d_lds + t * BN * STR, brow, lane);
          Mma<T>::mma(a, bd, acc[t][fm][fn]);
          if (SIGMA_MODE == 2) {
            auto be = Mma<T>::load(e_lds + t * BN * STR, brow, lane);
            Mma<T>::mma(a, be, sacc[t][fm][fn]);
          }
        }
      }
    }
    __syncthreads();

    if (--steps_left > 0 && ck + BK < nrows) continue;
    // block boundary (or the end): NSLICE noise draws and NSLICE unipolar
    // ADCs on the live fragments, shift-added; then the block's offset
    steps_left = steps_per_block;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        int64_t mb = xbar_frag_m(m0, wm, fm, lane);
        int n = xbar_frag_n(n0, wn, fn, lane);
#pragma unroll
        for (int t = 0; t < NSLICE; ++t) {
          const float shift = (float)(1 << (t * cell_bits));
          float g4[4] = {};
          if (SIGMA_MODE > 0)
            gauss4(seed,
                   (uint64_t)((((int64_t)b * NSLICE + t) * g.M + mb) * g.K + n),
                   g4);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            bool inside = mb + reg < g.M && n < g.K;
            float p = __fmul_rn(w_step, acc[t][fm][fn][reg]);
            float sig = 0.0f;
            if (SIGMA_MODE > 0) {
              sig = (SIGMA_MODE == 2)
                  ? __fadd_rn(__fmul_rn(w_step2, sacc[t][fm][fn][reg]), p)
                  : __fadd_rn(__fmul_rn(sq1, acc[t][fm][fn][reg]), p);
              sig = fmaxf(sig, 0.0f);
            }
            XbarPartial c = xbar_convert<SIGMA_MODE, ADC, true>(
                p, sig, g4[reg], factor, step, inv_step, qu);
            if (TELEM) {
              if (SIGMA_MODE > 0) {
                ntot[fm][fn][reg] += shift * c.noise;
                if (inside) t_sum_sigma += p;
              }
              if (ADC && inside && (c.t > qu || c.t < 0.0f)) t_sat += 1.0f;
              ycl[fm][fn][reg] += shift * p;
              if (inside) t_vmax = fmaxf(t_vmax, fabsf(c.v));
            }
            oacc[fm][fn][reg] += shift * c.q;
          }
          acc[t][fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          sacc[t][fm][fn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float off = __fmul_rn(w_min, xacc[fm][reg]);
          oacc[fm][fn][reg] = __fadd_rn(oacc[fm][fn][reg], off);
          if (TELEM) ycl[fm][fn][reg] = __fadd_rn(ycl[fm][fn][reg], off);
        }
      }
      xacc[fm] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    ++b;
  }

  xbar_finish<T, SIGMA_MODE, ADC, TELEM>(oacc, ycl, ntot, bias, out, g, m0, n0,
                                         wid, wm, wn, lane, t_sum_sigma, t_sat,
                                         t_vmax, telem, sat_count);
}

// ---------------------------------------------------------------------------
// Programming a layer's weight codes onto imperfect cells: one launch writes
// G[NSLICE][K][pitch] (digit units, the dtype of wq) for the PROG path above.
// For the weight matrix in crossbar-row order [K, n], slice t, column k, row i
//   code   = clamp(rint((f32(wq) - w_min) * inv_w_step), 0, 2^B - 1)
//   d_t    = (code >> tE) & (2^E - 1)
//   (u, z) = ONE Philox4x32 draw, key = chip seed, counter = (t*K + k)*n + i:
//            u = u01(word 0), z = Box-Muller on words 2, 3
//   d'_t   = 0 if u < p_off (stuck at the high-resistance state),
//            2^E - 1 else if u < p_off + p_on (stuck on), else d_t
//   G_t    = round_to_dtype(max(d'_t * (1 + sigma * z), 0))
// in fp32 with the one rounding. Multiplicative Gaussian variation clamped at
// zero: an off cell stays off, a stuck-on cell varies like any other.
// Log-normal variation and additive HRS leakage are not modelled. One thread
// owns a (k, i) and walks the slices; columns n..pitch-1 are written as zeros.
// ``fresh`` sends the seed through graph_seed, so a captured step programs a
// new chip on every replay; a fixed chip keeps the seed as given.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock)
void xbar_program_cells_kernel(const T* __restrict__ wq, T* __restrict__ G,
                               int K, int n, int pitch, int nslice,
                               int w_bits, int cell_bits,
                               const float* __restrict__ cell_p,
                               float sigma, float p_off, float p_on,
                               uint64_t seed, int fresh,
                               const int64_t* __restrict__ seed_base) {
  if (fresh) seed = graph_seed(seed_base, seed);
  int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (int64_t)K * pitch) return;
  int k = (int)(idx / pitch);
  int i = (int)(idx - (int64_t)k * pitch);
  const int64_t slice = (int64_t)K * pitch;
  if (i >= n) {
    for (int t = 0; t < nslice; ++t) G[t * slice + idx] = from_f32<T>(0.0f);
    return;
  }
  const float inv_w_step = cell_p[1];
  const float w_min = cell_p[2];
  const float code_max = (float)((1 << w_bits) - 1);
  const int dmask = (1 << cell_bits) - 1;
  const float p_any = __fadd_rn(p_off, p_on);
  int code = xbar_code(to_f32(wq[(int64_t)k * n + i]), w_min, inv_w_step,
                       code_max);
  for (int t = 0; t < nslice; ++t) {
    Philox4 p = philox4x32(seed, (uint64_t)(((int64_t)t * K + k) * n + i));
    float u = u01(p.x);
    float z = sqrtf(-2.0f * __logf(u01_open(p.z)))
        * __cosf(6.2831853071795864f * u01(p.w));
    float d = xbar_digit(code, t, cell_bits, dmask);
    if (u < p_off) d = 0.0f;
    else if (u < p_any) d = (float)dmask;
    float v = __fmul_rn(d, __fadd_rn(1.0f, __fmul_rn(sigma, z)));
    G[t * slice + idx] = from_f32<T>(fmaxf(v, 0.0f));
  }
}

// slice count of a bit-sliced-weight call, after checking w_bits / cell_bits
// / cell
int check_xbar_cells_args(int64_t w_bits, int64_t cell_bits,
                          const torch::Tensor& cell, const torch::Tensor& x,
                          const char* who) {
  TORCH_CHECK(cell_bits >= 1 && cell_bits <= 4, who,
              ": cell_bits must be 1..4, got ", cell_bits);
  TORCH_CHECK(w_bits >= 1 && w_bits <= 8, who, ": w_bits must be 1..8, got ",
              w_bits);
  int64_t slices = (w_bits + cell_bits - 1) / cell_bits;
  TORCH_CHECK(slices <= 4, who, ": w_bits ", w_bits, " at cell_bits ",
              cell_bits, " is ", slices, " slices, at most 4 are built; the "
              "smallest cell_bits that works is ", (w_bits + 3) / 4);
  TORCH_CHECK(cell.numel() == 3 && cell.scalar_type() == torch::kFloat32 &&
                  cell.is_contiguous() && cell.device() == x.device(),
              who, ": cell must be the fp32 device tensor "
              "[w_step, 1/w_step, w_min]");
  return (int)slices;
}

// x and wq2 are raw NHWC / [K, nrows] row-matrix views (no w_raw); out is
// allocated by the caller with M*K elements in [M, K] raw order
std::vector<torch::Tensor> xbar_cells_fwd_impl(
    const torch::Tensor& x, torch::Tensor wq2, const torch::Tensor& bias,
    ConvGeom g, torch::Tensor out, int64_t sigma_mode,
    const torch::Tensor& factor, int64_t xbar_rows, int64_t adc_bits,
    const torch::Tensor& adc, int64_t w_bits, int64_t cell_bits,
    const torch::Tensor& cell, int64_t seed, bool telem, const char* who,
    const torch::Tensor* cells = nullptr /* programmed conductances G */) {
  check_xbar_args(sigma_mode, xbar_rows, adc_bits, adc, x, who);
  const int NS = check_xbar_cells_args(w_bits, cell_bits, cell, x, who);
  check_xbar_weights(x, g, wq2, wq2, who);
  const int nrows = g.R * g.S * g.C;
  const int pitch = xbar_pitch(nrows, x.element_size());
  const bool prog = cells != nullptr;
  const bool padded = pitch != nrows;
  torch::Tensor gc;
  if (prog) {
    // G[T, K, n]: contiguous, or the view xbar_program_cells returns (rows
    // padded with zeros to a pitch of 8 elements), which is read in place
    const torch::Tensor& c = *cells;
    TORCH_CHECK(c.dim() == 3 && c.size(0) == NS && c.size(1) == g.K &&
                    c.size(2) == nrows,
                who, ": cells must have the shape [", NS, ", ", g.K, ", ",
                nrows, "] (slices, output columns, crossbar rows), got ",
                c.sizes());
    TORCH_CHECK(c.scalar_type() == x.scalar_type(), who,
                ": cells must have the dtype of x");
    TORCH_CHECK(c.device() == x.device(), who,
                ": cells must be on the device of x");
    // (the padding must be inside the view's storage: the kernel reads it)
    const bool pitched =
        padded && c.stride(2) == 1 && c.stride(1) == pitch &&
        c.stride(0) == (int64_t)g.K * pitch &&
        (c.storage_offset() + (int64_t)NS * g.K * pitch) * c.element_size() <=
            (int64_t)c.storage().nbytes();
    TORCH_CHECK(c.is_contiguous() || pitched, who,
                ": cells must be contiguous (or the row-padded view that "
                "xbar_program_cells returns)");
    // the 16-bit spans are 16-byte vector loads
    const bool aligned = ((uintptr_t)c.data_ptr() & 15) == 0;
    gc = c;
    if (padded && !(pitched && aligned))
      gc = at::constant_pad_nd(c, {0, pitch - nrows}, 0).contiguous();
    else if (!aligned)
      gc = c.clone();
  } else {
    wq2 = pad_rows8(wq2, nrows, x.element_size());
  }
  XbarLaunch L(x, bias, g, factor, adc_bits, adc, telem, who);
  float qu = L.adc_on ? (float)((1 << adc_bits) - 1) : 0.0f;   // unipolar
  // one-bit digits are their own squares: abs2 runs on the abs instantiation
  // (not on programmed cells: G^2 != G)
  const int fold = (sigma_mode == 2 && cell_bits == 1 && !prog) ? 1 : 0;
  const int64_t kmode = fold ? 1 : sigma_mode;
  NN_DISPATCH(x.scalar_type(), "xbar_cells_fwd", [&] {
    using T = typename DevT<scalar_t>::type;
    // x tile + NS digit tiles (+ NS tiles of squares with abs2): at most
    // (64 + 8 * 64) * 80 = 46080 bytes for the 16-bit dtypes; fp32 with
    // four slices and abs2 is 82944 bytes and opts in to the large LDS
    size_t lds = (size_t)(BM + (kmode == 2 ? 2 : 1) * NS * BN)
        * Mma<T>::STRIDE;
    auto stream = c10::hip::getCurrentHIPStream();
    const T* xp = (const T*)x.data_ptr();
    const T* wqp = (const T*)wq2.data_ptr();
    T* op = (T*)out.data_ptr();
    const float* cp = cell.data_ptr<float>();
    const T* gp = prog ? (const T*)gc.data_ptr() : nullptr;
    const int64_t gstride = (int64_t)g.K * pitch;
    uint64_t sd = (uint64_t)seed;
    using TT = std::true_type; using FF = std::false_type;
    dispatch_slices(NS, [&](auto ns) {
      xbar_dispatch_mode(kmode, L.adc_on, telem,
                         [&](auto sm, auto ad, auto tl) {
        auto launch = [&](auto pg) {
          auto kfn = xbar_cells_fwd_kernel<T, decltype(ns)::value,
                                           decltype(sm)::value,
                                           decltype(ad)::value,
                                           decltype(tl)::value,
                                           decltype(pg)::value>;
          if (lds > 65536)
            TORCH_CHECK(hipFuncSetAttribute(
                            (const void*)kfn,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) == hipSuccess,
                        who, ": ", lds, " bytes of LDS are not available");
          hipLaunchKernelGGL(kfn, L.grid, dim3(kBlock), lds, stream, xp, wqp,
                             L.bias, op, g, pitch, (int)xbar_rows,
                             (int)w_bits, (int)cell_bits, fold, cp, L.factor,
                             L.adc, qu, sd, L.telem, L.sat_count, g_seed_base,
                             gp, gstride);
        };
        if (prog) launch(TT{}); else launch(FF{});
      });
    });
  });
  return L.finish(out);
}

}  // namespace

// bit-sliced weights (w_bits-bit offset-binary codes on the grid
// w_min + code * w_step, cell_bits per column); cell = fp32
// [w_step, 1/w_step, w_min]; adc is [step, 1/step] of the unipolar step
// adc_max / (2^bits - 1)
std::vector<torch::Tensor> xbar_cells_fwd_conv(
    torch::Tensor x, torch::Tensor wq, torch::Tensor bias, int64_t stride,
    int64_t pad, int64_t sigma_mode, torch::Tensor factor, int64_t xbar_rows,
    int64_t adc_bits, torch::Tensor adc, int64_t w_bits, int64_t cell_bits,
    torch::Tensor cell, int64_t seed, bool telem) {
  const char* who = "xbar_cells_fwd_conv";
  XbarConv cv(x, wq, nullptr, stride, pad, who);
  return xbar_cells_fwd_impl(x, cv.rows(wq), bias, cv.g, cv.out, sigma_mode,
                             factor, xbar_rows, adc_bits, adc, w_bits,
                             cell_bits, cell, seed, telem, who);
}

std::vector<torch::Tensor> xbar_cells_fwd_linear(
    torch::Tensor x, torch::Tensor wq, torch::Tensor bias, int64_t sigma_mode,
    torch::Tensor factor, int64_t xbar_rows, int64_t adc_bits,
    torch::Tensor adc, int64_t w_bits, int64_t cell_bits, torch::Tensor cell,
    int64_t seed, bool telem) {
  const char* who = "xbar_cells_fwd_linear";
  TORCH_CHECK(wq.dim() == 2 && wq.size(1) == x.size(1), who,
              ": weight shape mismatch");
  auto g = linear_geom(x, wq.size(0));
  auto out = torch::empty({x.size(0), wq.size(0)}, x.options());
  return xbar_cells_fwd_impl(x, wq, bias, g, out, sigma_mode, factor,
                             xbar_rows, adc_bits, adc, w_bits, cell_bits,
                             cell, seed, telem, who);
}

// the same on programmed cells: ``cells`` = G[T, K, n] of
// xbar_program_cells (digit units, the dtype of x) stands in for the digits;
// wq gives the geometry only
std::vector<torch::Tensor> xbar_prog_fwd_conv(
    torch::Tensor x, torch::Tensor wq, torch::Tensor cells, torch::Tensor bias,
    int64_t stride, int64_t pad, int64_t sigma_mode, torch::Tensor factor,
    int64_t xbar_rows, int64_t adc_bits, torch::Tensor adc, int64_t w_bits,
    int64_t cell_bits, torch::Tensor cell, int64_t seed, bool telem) {
  const char* who = "xbar_prog_fwd_conv";
  XbarConv cv(x, wq, nullptr, stride, pad, who);
  return xbar_cells_fwd_impl(x, cv.rows(wq), bias, cv.g, cv.out, sigma_mode,
                             factor, xbar_rows, adc_bits, adc, w_bits,
                             cell_bits, cell, seed, telem, who, &cells);
}

std::vector<torch::Tensor> xbar_prog_fwd_linear(
    torch::Tensor x, torch::Tensor wq, torch::Tensor cells, torch::Tensor bias,
    int64_t sigma_mode, torch::Tensor factor, int64_t xbar_rows,
    int64_t adc_bits, torch::Tensor adc, int64_t w_bits, int64_t cell_bits,
    torch::Tensor cell, int64_t seed, bool telem) {
  const char* who = "xbar_prog_fwd_linear";
  TORCH_CHECK(wq.dim() == 2 && wq.size(1) == x.size(1), who,
              ": weight shape mismatch");
  auto g = linear_geom(x, wq.size(0));
  auto out = torch::empty({x.size(0), wq.size(0)}, x.options());
  return xbar_cells_fwd_impl(x, wq, bias, g, out, sigma_mode, factor,
                             xbar_rows, adc_bits, adc, w_bits, cell_bits,
                             cell, seed, telem, who, &cells);
}

// program a layer's weight codes onto imperfect cells (see
// xbar_program_cells_kernel): wq is a channels-last conv filter [K, C, R, S]
// (rows in the (r, s, c) order of xbar_cells_fwd_conv) or a linear weight
// [K, n]. Returns G[T, K, n]; for the 16-bit dtypes the rows sit at a pitch
// padded to 8 elements and the result is that view.
torch::Tensor xbar_program_cells(torch::Tensor wq, int64_t w_bits,
                                 int64_t cell_bits, torch::Tensor cell,
                                 double sigma, double p_stuck_off,
                                 double p_stuck_on, int64_t seed, bool fresh) {
  const char* who = "xbar_program_cells";
  TORCH_CHECK(wq.is_cuda(), who, ": wq must be a GPU tensor");
  const int NS = check_xbar_cells_args(w_bits, cell_bits, cell, wq, who);
  TORCH_CHECK(sigma >= 0.0, who, ": sigma must be >= 0, got ", sigma);
  TORCH_CHECK(p_stuck_off >= 0.0, who, ": p_stuck_off must be >= 0, got ",
              p_stuck_off);
  TORCH_CHECK(p_stuck_on >= 0.0, who, ": p_stuck_on must be >= 0, got ",
              p_stuck_on);
  TORCH_CHECK(p_stuck_off + p_stuck_on <= 1.0, who,
              ": p_stuck_off + p_stuck_on must be <= 1, got ",
              p_stuck_off + p_stuck_on);
  TORCH_CHECK(wq.dim() == 2 || wq.dim() == 4, who,
              ": wq must be a [K, n] or a [K, C, R, S] tensor");
  torch::Tensor wq2;
  if (wq.dim() == 4) {
    check_cl(wq, "xbar_program_cells wq");
    wq2 = wq.permute({0, 2, 3, 1}).reshape({wq.size(0), -1}).contiguous();
  } else {
    wq2 = wq.contiguous();
  }
  const int64_t K = wq2.size(0), n = wq2.size(1);
  TORCH_CHECK(K > 0 && n > 0 && (int64_t)NS * K * (n + 7) < (1ll << 31), who,
              ": wq is empty or too large");
  const int64_t pitch = xbar_pitch((int)n, wq2.element_size());
  auto G = torch::empty({(int64_t)NS, K, pitch}, wq2.options());
  const int64_t total = K * pitch;
  NN_DISPATCH(wq2.scalar_type(), "xbar_program_cells", [&] {
    using T = typename DevT<scalar_t>::type;
    auto stream = c10::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(xbar_program_cells_kernel<T>,
                       dim3((unsigned)((total + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, stream, (const T*)wq2.data_ptr(),
                       (T*)G.data_ptr(), (int)K, (int)n, (int)pitch, NS,
                       (int)w_bits, (int)cell_bits, cell.data_ptr<float>(),
                       (float)sigma, (float)p_stuck_off, (float)p_stuck_on,
                       (uint64_t)seed, fresh ? 1 : 0, g_seed_base);
  });
  HIP_CHECK_LAST();
  return pitch == n ? G : G.narrow(2, 0, n);
}
