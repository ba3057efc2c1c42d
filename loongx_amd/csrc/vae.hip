// vae.hip -- row kernels of the FLUX VAE (diffusers AutoencoderKL; reference call sites src/flux/generate.py:375-380 decode,
// src/flux/pipeline_tools.py:7-30 encode) for gfx950. The VAE sits either side of the denoise loop; its
// convolutions run as implicit GEMMs on the DiT's MFMA kernel (lx_gemm_bf16: im2col rows x [Cout, 9 Cin] weights, fused
// bias / fp32 residual epilogues), so what lives here is the HBM-bound glue in NHWC layout, each piece ONE kernel body:
//   * GroupNorm(32 groups, eps, affine) [+ SiLU]: partial sums per (image, row chunk, group), then one normalising pass;
//   * im2col for 3x3 convolutions: pad 1 / stride 1, the encoder's stride-2 downsample with its (0,1,0,1) padding, and the
//     decoder's nearest-neighbour 2x upsample folded into the gather (the upsampled image is never materialised);
//   * row softmax (fp32 scores -> 16-bit probabilities) for the single-head mid-block attention, over the first n_valid columns of a key
//     axis padded to the GEMM's granule (token counts that are no multiple of 64): the pad keys get probability +0.
// The operand format of the GEMM that consumes an image is a STORE POLICY of these bodies (Fmt*, below), not a kernel of its own:
//   bf16   the default;
//   fp16   the operand images of LX_OPERANDS_F16 launches (LxAutoencoderKL(operands="fp16")); GroupNorm and lx_convert_f16 saturate at
//          +-65504 and count the waves that clipped;
//   pair   precise mode: x as hi = bf16(x) at column c and lo = bf16(x - hi) at column lo_off + c of the same row (split_bf16_pair), the
//          operand of a k_segs = 2 | 3 launch of lx_gemm_bf16. The residual stream between the GEMMs stays fp32.
// A single 16-bit image is the pair layout without a lo half. im2col moves 16-bit words whatever they hold: its template counts halves.
// A new format is one more policy struct, one instantiation per kernel in the launch routines and one entry point per kernel.
// All accesses are 8-16 B per lane along the channel axis (im2col and the softmax fall back to scalar ones where the rows do not allow it).
#include "common.h"

namespace {

// ---- store policies ----------------------------------------------------------------------------------------------------------
// pack2 / one: two / one fp32 values in the 16-bit format. kPair: there is a lo half. report: tell the caller's overflow word.
struct FmtBf16 {
  static constexpr bool kPair = false;
  __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
  __device__ __forceinline__ uint16_t one(float v) { return f32_to_bf16(v); }
  __device__ __forceinline__ void report(int*) {}
};
// fp16 of values known to fit: probabilities are <= 1, so there is no saturation and no overflow to report
struct FmtF16 {
  static constexpr bool kPair = false;
  __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    const f16x2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, v);
  }
  __device__ __forceinline__ uint16_t one(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
  __device__ __forceinline__ void report(int*) {}
};
// fp16 of anything: round to nearest even, saturated to +-65504; a wave that clipped a value adds 1 to *f16_ovf (NULL: not reported)
struct FmtF16Sat {
  static constexpr bool kPair = false;
  float mx = 0.f;
  __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack_op16x2<true>(lo, hi, mx); }
  __device__ __forceinline__ void report(int* f16_ovf) { report_f16_overflow(mx, f16_ovf); }
};
struct FmtPair {
  static constexpr bool kPair = true;
  __device__ __forceinline__ void report(int*) {}
};

// o[0..3] -> p[0..3] (and p[lo_off ..] of a pair), 8-byte stores; one value -> p[0]; +0 likewise
template <typename Fmt>
__device__ __forceinline__ void store4(Fmt& f, uint16_t* p, int lo_off, const float (&o)[4]) {
  if constexpr (Fmt::kPair) {
    uint16_t hh[4], ll[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) split_bf16_pair(o[k], hh[k], ll[k]);
    *(u32x2*)p = u32x2{pack_u16x2(hh[0], hh[1]), pack_u16x2(hh[2], hh[3])};
    *(u32x2*)(p + lo_off) = u32x2{pack_u16x2(ll[0], ll[1]), pack_u16x2(ll[2], ll[3])};
  } else {
    *(u32x2*)p = u32x2{f.pack2(o[0], o[1]), f.pack2(o[2], o[3])};
  }
}
template <typename Fmt>
__device__ __forceinline__ void store1(Fmt& f, uint16_t* p, int lo_off, float v) {
  if constexpr (Fmt::kPair) split_bf16_pair(v, p[0], p[lo_off]);
  else p[0] = f.one(v);
}
template <typename Fmt>
__device__ __forceinline__ void zero4(uint16_t* p, int lo_off) {
  *(u32x2*)p = u32x2{0u, 0u};
  if constexpr (Fmt::kPair) *(u32x2*)(p + lo_off) = u32x2{0u, 0u};
}
template <typename Fmt>
__device__ __forceinline__ void zero1(uint16_t* p, int lo_off) {
  p[0] = 0;
  if constexpr (Fmt::kPair) p[lo_off] = 0;
}

// ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
// x: [B, P, C] (P = H*W pixels), fp32 or bf16. Pass 1: block (chunk, b) sums its rows per channel in registers, folds channels
// into groups through LDS, writes part[b][chunk][g] = (sum, sumsq). Pass 2 re-reduces the few partials per group on the fly.
template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <>
__device__ __forceinline__ f32x4 load4<uint16_t>(const uint16_t* p) {
  const u32x2 r = *(const u32x2*)p;
  return f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
}

// The pair format's statistics: mean of group g's channels at pixel 0 of the image (x0). A sample of the group, so |mean - shift| is of the
// order of the spread and E[d^2] - E[d]^2 cancels nothing to speak of, however large the mean is against the spread.
__device__ __forceinline__ float gn_shift(const float* __restrict__ x0, int g, int cpg) {
  float s = 0.f;
  for (int j = 0; j < cpg; ++j) s += x0[g * cpg + j];
  return s / (float)cpg;
}

// SHIFT: the sums are taken of x - gn_shift (fp32 x only).
template <typename T, bool SHIFT>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, int P, int C, int G, int rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[2][256];                         // every thread's (sum, sumsq); folded per group in a FIXED order (no atomics)
  const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
  const int lanes_per_row = C / 4, rows_per_iter = 256 / lanes_per_row, cpg = C / G;
  const int tid = threadIdx.x, c4 = (tid % lanes_per_row) * 4, rsub = tid / lanes_per_row;
  const int r0 = chunk * rows_per_chunk, r1 = min(P, r0 + rows_per_chunk);
  const T* x0 = x + (size_t)b * P * C;
  float sh = 0.f;                                       // the thread's 4 channels lie in ONE group (C/G >= 4, multiple of 4)
  if constexpr (SHIFT) sh = gn_shift(x0, c4 / cpg, cpg);
  float s = 0.f, q = 0.f;
  const T* xb = x0 + c4;
  for (int r = r0 + rsub; r < r1; r += rows_per_iter) {
    f32x4 v = load4<T>(xb + (size_t)r * C);
    if constexpr (SHIFT) {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] -= sh;
    }
    s += (v[0] + v[1]) + (v[2] + v[3]);
    q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  red[0][tid] = s;
  red[1][tid] = q;
  __syncthreads();
  if (tid < G) {
    const int lpg = cpg / 4;                            // lanes per group within a row
    float ss = 0.f, qq = 0.f;
    for (int rs = 0; rs < rows_per_iter; ++rs)
      for (int j = 0; j < lpg; ++j) {
        const int t = rs * lanes_per_row + tid * lpg + j;
        ss += red[0][t];
        qq += red[1][t];
      }
    float* o = part + (((size_t)b * nchunk + chunk) * G + tid) * 2;
    o[0] = ss;
    o[1] = qq;
  }
}

// y: rows of ldy elements, one per pixel (a single image: ldy = C). The partials become (mean, rstd) in fp32 for the single images; for the
// pair they are those of gn_stats_kernel<float, true> and are combined, and the variance formed, in double, with the shift added back.
template <typename T, typename Fmt>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, int P, int C, int G, const float* __restrict__ part, int nchunk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int silu,
                                                       uint16_t* __restrict__ y, int ldy, int y_lo_off, int* __restrict__ f16_ovf) {
  const int b = blockIdx.y;
  const int cpg = C / G, c4s = C / 4;
  const size_t n4 = (size_t)P * c4s;
  const T* x0 = x + (size_t)b * P * C;
  Fmt fmt;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int c4 = (int)(i % c4s) * 4;
    const size_t p = i / c4s;
    const int g = c4 / cpg;
    const float* pp = part + ((size_t)b * nchunk * G + g) * 2;       // chunk k's partial: pp[k * G * 2]
    float mean, rstd;
    if constexpr (Fmt::kPair) {
      const double inv_n = 1.0 / ((double)P * (double)cpg);
      double s = 0.0, q = 0.0;
      for (int k = 0; k < nchunk; ++k) {
        s += (double)pp[(size_t)k * G * 2];
        q += (double)pp[(size_t)k * G * 2 + 1];
      }
      const double md = s * inv_n;                          // mean - shift
      rstd = (float)(1.0 / sqrt(fmax(q * inv_n - md * md, 0.0) + (double)eps));
      mean = (float)((double)gn_shift(x0, g, cpg) + md);
    } else {
      const float inv_n = 1.0f / ((float)P * (float)cpg);
      float s = 0.f, q = 0.f;
      for (int k = 0; k < nchunk; ++k) {
        s += pp[(size_t)k * G * 2];
        q += pp[(size_t)k * G * 2 + 1];
      }
      mean = s * inv_n;
      rstd = rsqrtf(fmaxf(q * inv_n - mean * mean, 0.f) + eps);
    }
    const f32x4 v = load4<T>(x0 + i * 4);
    const f32x4 ga = *(const f32x4*)(gamma + c4), be = *(const f32x4*)(beta + c4);
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t = (v[c] - mean) * rstd * ga[c] + be[c];
      if (silu) t = t / (1.0f + __expf(-t));
      o[c] = t;
    }
    store4(fmt, y + ((size_t)b * P + p) * ldy + c4, y_lo_off, o);
  }
  fmt.report(f16_ovf);
}

// ---- im2col for 3x3 convolutions, NHWC 16-bit words -> [B*Ho*Wo, NH * Kpad], column = half * Kpad + (dy*3 + dx)*C + c ---------------------
// mode 0: stride 1, pad 1 (Ho = H, Wo = W);  mode 1: stride 2, pad (0,1,0,1) (Ho = H/2, Wo = W/2: diffusers Downsample2D with padding=0);
// mode 2: nearest 2x upsample, then stride 1 pad 1 (Ho = 2H, Wo = 2W: Upsample2D + its conv). Columns >= 9*C of a half are zero padding.
// NH = 1: a single image, ldx = C. NH = 2: a pair image, pixel rows [hi C | ... | lo C] (stride ldx, lo at x_lo_off) -> rows
// [hi taps Kpad | lo taps Kpad]. A work item is (output pixel, half, tap, VEC ? 8 channels : 1 channel); the halves are gathered independently.
template <bool VEC, int NH>
__global__ __launch_bounds__(256) void im2col3x3_kernel(const uint16_t* __restrict__ x, int ldx, int x_lo_off, int B, int H, int W, int C, int mode,
                                                        uint16_t* __restrict__ out, int Kpad) {
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  constexpr int cv = VEC ? 8 : 1;                          // channels per work item
  const int per_tap = C / cv;
  const size_t rows = (size_t)B * Ho * Wo, items = rows * (9 * NH) * per_tap;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const int cc = (int)(i % per_tap) * cv;
    size_t r = i / per_tap;
    const int tap = (int)(r % 9);
    r /= 9;
    const int half = (int)(r % NH);
    r /= NH;                                               // output pixel index (b, yo, xo)
    const int xo = (int)(r % Wo), yo = (int)((r / Wo) % Ho), b = (int)(r / ((size_t)Wo * Ho));
    const int dy = tap / 3, dx = tap % 3;
    int yi, xi;
    bool ok;
    if (mode == 1) { yi = 2 * yo + dy; xi = 2 * xo + dx; ok = yi < H && xi < W; }
    else if (mode == 2) { const int yu = yo + dy - 1, xu = xo + dx - 1; ok = yu >= 0 && yu < Ho && xu >= 0 && xu < Wo; yi = yu >> 1; xi = xu >> 1; }
    else { yi = yo + dy - 1; xi = xo + dx - 1; ok = yi >= 0 && yi < H && xi >= 0 && xi < W; }
    uint16_t* o = out + (r * NH + half) * Kpad + tap * C + cc;
    const uint16_t* s = x + (((size_t)b * H + (ok ? yi : 0)) * W + (ok ? xi : 0)) * ldx + half * x_lo_off + cc;
    if (VEC) *(u32x4*)o = ok ? *(const u32x4*)s : u32x4{0u, 0u, 0u, 0u};
    else *o = ok ? *s : (uint16_t)0;
  }
  // zero the K padding (columns [9C, Kpad) of every half)
  const int padc = Kpad - 9 * C;
  if (padc > 0) {
    const size_t n = rows * NH * padc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
      out[(i / padc) * Kpad + 9 * C + (i % padc)] = 0;      // i / padc = NH * row + half, and a half is Kpad columns
  }
}

// ---- row softmax over the first n_valid columns of a row whose key axis is padded: P[row, 0:n_valid] = softmax(scale * S[row, 0:n_valid]),
// P[row, n_valid:n_store] = +0; a pair has its lo half at P[row, p_lo_off + c], pad columns included. One wave per row. Columns >= n_valid
// of S (scores against padding: anything, NaN included) are never loaded; nothing at or beyond column n_store of a half is written.
// VEC: every row of S starts 16-byte and every row of P (and its lo half) 8-byte aligned, so columns [0, n_valid & ~3) go four per lane
// and only the < 4 columns behind them one per lane; otherwise every access is a scalar one.
template <bool VEC, typename Fmt>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, int lds, float scale, uint16_t* __restrict__ Pm, int ldp,
                                                           int p_lo_off, int M, int n_valid, int n_store) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* s = S + (size_t)row * lds;
  uint16_t* p = Pm + (size_t)row * ldp;
  Fmt fmt;
  const int nv = VEC ? (n_valid & ~3) : 0;                // [0, nv) in vectors, [nv, n_valid) one column per lane
  float m = -INFINITY;
  for (int c = lane * 4; c < nv; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
    m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  }
  for (int c = nv + lane; c < n_valid; c += 64) m = fmaxf(m, s[c]);
  m = wave_max(m) * scale;
  float l = 0.f;
  for (int c = lane * 4; c < nv; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) l += __expf(v[k] * scale - m);
  }
  for (int c = nv + lane; c < n_valid; c += 64) l += __expf(s[c] * scale - m);
  const float inv = 1.0f / wave_sum(l);
  for (int c = lane * 4; c < nv; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __expf(v[k] * scale - m) * inv;
    store4(fmt, p + c, p_lo_off, o);
  }
  for (int c = nv + lane; c < n_valid; c += 64) store1(fmt, p + c, p_lo_off, __expf(s[c] * scale - m) * inv);
  // the pad keys' probabilities: scalar up to the next multiple of 4 (z0), vectors up to the last one (z1), scalar to n_store
  const int z0 = VEC ? min((n_valid + 3) & ~3, n_store) : n_store, z1 = VEC ? max(z0, n_store & ~3) : n_store;
  for (int c = n_valid + lane; c < z0; c += 64) zero1<Fmt>(p + c, p_lo_off);
  for (int c = z0 + lane * 4; c < z1; c += 256) zero4<Fmt>(p + c, p_lo_off);
  for (int c = z1 + lane; c < n_store; c += 64) zero1<Fmt>(p + c, p_lo_off);
}

// ---- fp32 | bf16 -> the fp16 operand image, saturated to +-65504 AND counted (lx_convert's dst 2 clips silently). NaN stays NaN.
__global__ __launch_bounds__(256) void convert_f16_kernel(uint16_t* __restrict__ dst, const void* __restrict__ src, int src_bf16, size_t n,
                                                          int* __restrict__ f16_ovf) {
  const size_t stride = (size_t)gridDim.x * 256;
  float mx = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float v = src_bf16 ? bf16_to_f32(((const uint16_t*)src)[i]) : ((const float*)src)[i];
    const uint16_t h = (uint16_t)(pack_f16x2_sat(v, 0.f, mx) & 0xffffu);
    dst[i] = v != v ? (uint16_t)0x7e00u : h;               // (the clamp would turn a NaN into -65504)
  }
  report_f16_overflow(mx, f16_ovf);
}

// ---- host side: one argument check and one launch routine per kernel family; the entry points say which of the checks apply to them ------
int gn_chunks(int P) { return P >= 4096 ? 64 : (P >= 256 ? 16 : 1); }

struct GnCall {
  const void* x;
  int B, P, C, G;
  const float *gamma, *beta;
  float eps;
  int silu;
  void* y;
  int ldy, y_lo_off;                                      // a single image: C, 0
  void* ws;
  size_t ws_bytes;
  int32_t* f16_ovf;
  void* stream;
};

// pair: y is a pair image (its layout is checked). aligned: the operands' alignment is checked (lx_groupnorm_silu never asked for it).
int gn_check(const char* name, const GnCall& a, bool pair, bool aligned) {
  const int C = a.C, G = a.G;
  LX_CHECK_ARG(a.x && a.y && a.gamma && a.beta && a.ws, "%s: NULL operand", name);
  LX_CHECK_ARG(a.B > 0 && a.P > 0 && C > 0 && G > 0 && G <= 64 && C % G == 0 && (C / G) % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "%s: need G <= 64, C %% G == 0, (C/G) %% 4 == 0, C/4 a divisor of 256 (C=%d G=%d)", name, C, G);
  if (pair) LX_CHECK_ARG(a.y_lo_off % 8 == 0 && a.y_lo_off >= C && a.ldy % 4 == 0 && a.ldy >= a.y_lo_off + C, "%s: need y_lo_off %% 8 == 0, C <= y_lo_off, y_lo_off + C <= ldy, ldy %% 4 == 0 (C=%d ldy=%d y_lo_off=%d)", name, C, a.ldy, a.y_lo_off);
  if (aligned) LX_CHECK_ARG(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.y & 7) == 0 && ((uintptr_t)a.gamma & 15) == 0 && ((uintptr_t)a.beta & 15) == 0 && ((uintptr_t)a.f16_ovf & 3) == 0, "%s: misaligned operand", name);
  LX_CHECK_ARG(a.ws_bytes >= lx_groupnorm_workspace_bytes(a.B, a.P, G), "%s: workspace too small", name);
  return LX_OK;
}

// The two passes (arguments checked by the caller).
template <typename T, typename Fmt>
int gn_launch(const char* name, const GnCall& a) {
  const int nchunk = gn_chunks(a.P), rpc = (a.P + nchunk - 1) / nchunk;
  float* part = (float*)a.ws;
  const size_t n4 = (size_t)a.P * a.C / 4;
  const int gx = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipStream_t s = (hipStream_t)a.stream;
  hipLaunchKernelGGL((gn_stats_kernel<T, Fmt::kPair>), dim3(nchunk, a.B), dim3(256), 0, s, (const T*)a.x, a.P, a.C, a.G, rpc, part);
  hipLaunchKernelGGL((gn_apply_kernel<T, Fmt>), dim3(gx, a.B), dim3(256), 0, s, (const T*)a.x, a.P, a.C, a.G, part, nchunk, a.gamma, a.beta, a.eps, a.silu,
                     (uint16_t*)a.y, a.ldy, a.y_lo_off, (int*)a.f16_ovf);
  LX_LAUNCH_CHECK(name);
  return LX_OK;
}

// NH = 2: x is a pair image (its layout is checked). vec: the caller's word on whether 16-byte items are possible.
template <int NH>
int im2col_run(const char* name, const void* x, int ldx, int x_lo_off, int B, int H, int W, int C, int mode, void* out, int Kpad, bool vec, void* stream) {
  LX_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && C > 0, "%s: bad arguments", name);
  LX_CHECK_ARG(mode >= 0 && mode <= 2 && (mode != 1 || (H % 2 == 0 && W % 2 == 0)), "%s: mode 0|1|2 (mode 1 needs even H, W)", name);
  LX_CHECK_ARG(Kpad >= 9 * C && Kpad % 8 == 0, "%s: Kpad=%d must be >= 9*C and a multiple of 8", name, Kpad);
  if (NH == 2) LX_CHECK_ARG(x_lo_off % 8 == 0 && x_lo_off >= C && ldx >= x_lo_off + C, "%s: need x_lo_off %% 8 == 0 and C <= x_lo_off, x_lo_off + C <= ldx (C=%d ldx=%d x_lo_off=%d)", name, C, ldx, x_lo_off);
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  const size_t items = (size_t)B * Ho * Wo * (9 * NH) * (vec ? C / 8 : C);
  const int grid = (int)((items + 255) / 256 < 16384 ? (items + 255) / 256 : 16384);
  auto* kernel = vec ? im2col3x3_kernel<true, NH> : im2col3x3_kernel<false, NH>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, x_lo_off, B, H, W, C, mode, (uint16_t*)out, Kpad);
  LX_LAUNCH_CHECK(name);
  return LX_OK;
}

struct SoftmaxCall {
  const float* S;
  int lds;
  float scale;
  void* P;
  int ldp, p_lo_off;                                      // a single image: p_lo_off = 0
  int M, n_valid, n_store;
  void* stream;
};

// pair: P is a pair image (the leading-dimension line is the pair's). aligned: element alignment of S and P is checked (the fp16 form's line).
int softmax_check(const char* name, const SoftmaxCall& a, bool pair, bool aligned) {
  LX_CHECK_ARG(a.S && a.P, "%s: NULL operand", name);
  LX_CHECK_ARG(a.M > 0 && a.n_valid >= 1 && a.n_store >= a.n_valid, "%s: need M > 0 and 1 <= n_valid <= n_store (M=%d n_valid=%d n_store=%d)", name, a.M, a.n_valid, a.n_store);
  if (pair) LX_CHECK_ARG(a.lds >= a.n_valid && a.p_lo_off % 8 == 0 && a.p_lo_off >= a.n_store && a.ldp >= a.p_lo_off + a.n_store, "%s: need lds >= n_valid, p_lo_off %% 8 == 0 and n_store <= p_lo_off, p_lo_off + n_store <= ldp (lds=%d ldp=%d p_lo_off=%d n_valid=%d n_store=%d)", name, a.lds, a.ldp, a.p_lo_off, a.n_valid, a.n_store);
  else LX_CHECK_ARG(a.lds >= a.n_valid && a.ldp >= a.n_store, "%s: need lds >= n_valid and ldp >= n_store (lds=%d ldp=%d n_valid=%d n_store=%d)", name, a.lds, a.ldp, a.n_valid, a.n_store);
  if (aligned) LX_CHECK_ARG(((uintptr_t)a.S & 3) == 0 && ((uintptr_t)a.P & 1) == 0, "%s: misaligned operand", name);
  return LX_OK;
}

bool softmax_vec(const SoftmaxCall& a) { return ((uintptr_t)a.S & 15) == 0 && a.lds % 4 == 0 && ((uintptr_t)a.P & 7) == 0 && a.ldp % 4 == 0; }

template <typename Fmt>
int softmax_launch(const char* name, const SoftmaxCall& a, bool vec) {
  auto* kernel = vec ? softmax_rows_kernel<true, Fmt> : softmax_rows_kernel<false, Fmt>;
  hipLaunchKernelGGL(kernel, dim3((a.M + 3) / 4), dim3(256), 0, (hipStream_t)a.stream, a.S, a.lds, a.scale, (uint16_t*)a.P, a.ldp, a.p_lo_off, a.M, a.n_valid, a.n_store);
  LX_LAUNCH_CHECK(name);
  return LX_OK;
}

template <typename Fmt>
int softmax_run(const char* name, const SoftmaxCall& a, bool aligned) {
  const int rc = softmax_check(name, a, Fmt::kPair, aligned);
  return rc != LX_OK ? rc : softmax_launch<Fmt>(name, a, softmax_vec(a));
}

}  // namespace

extern "C" size_t lx_groupnorm_workspace_bytes(int B, int P, int G) { return (size_t)B * gn_chunks(P) * G * 2 * sizeof(float); }

extern "C" int lx_groupnorm_silu(const void* x, int x_is_bf16, int B, int P, int C, int G, const float* gamma, const float* beta, float eps,
                                 int silu, void* y, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "lx_groupnorm_silu";
  const GnCall a{x, B, P, C, G, gamma, beta, eps, silu, y, C, 0, ws, ws_bytes, nullptr, stream};
  const int rc = gn_check(name, a, false, false);
  if (rc != LX_OK) return rc;
  return x_is_bf16 ? gn_launch<uint16_t, FmtBf16>(name, a) : gn_launch<float, FmtBf16>(name, a);
}

extern "C" int lx_groupnorm_silu_f16(const float* x, int B, int P, int C, int G, const float* gamma, const float* beta, float eps, int silu, void* y,
                                     void* ws, size_t ws_bytes, int32_t* f16_ovf, void* stream) {
  const char* name = "lx_groupnorm_silu_f16";
  const GnCall a{x, B, P, C, G, gamma, beta, eps, silu, y, C, 0, ws, ws_bytes, f16_ovf, stream};
  const int rc = gn_check(name, a, false, true);
  return rc != LX_OK ? rc : gn_launch<float, FmtF16Sat>(name, a);
}

extern "C" int lx_groupnorm_silu_split(const float* x, int B, int P, int C, int G, const float* gamma, const float* beta, float eps, int silu,
                                       void* y, int ldy, int y_lo_off, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "lx_groupnorm_silu_split";
  const GnCall a{x, B, P, C, G, gamma, beta, eps, silu, y, ldy, y_lo_off, ws, ws_bytes, nullptr, stream};
  const int rc = gn_check(name, a, true, true);
  return rc != LX_OK ? rc : gn_launch<float, FmtPair>(name, a);
}

extern "C" int lx_im2col3x3(const void* x, int B, int H, int W, int C, int mode, void* out, int Kpad, void* stream) {
  return im2col_run<1>("lx_im2col3x3", x, C, 0, B, H, W, C, mode, out, Kpad, C % 8 == 0, stream);
}

extern "C" int lx_im2col3x3_split(const void* x, int ldx, int x_lo_off, int B, int H, int W, int C, int mode, void* out, int Kpad, void* stream) {
  const bool vec = C % 8 == 0 && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  return im2col_run<2>("lx_im2col3x3_split", x, ldx, x_lo_off, B, H, W, C, mode, out, Kpad, vec, stream);
}

// Every column a key, N % 4 == 0: the vector form of the one body, without an alignment test (this entry point never had one).
extern "C" int lx_softmax_rows(const float* S, int lds, float scale, void* P, int ldp, int M, int N, void* stream) {
  LX_CHECK_ARG(S && P && M > 0 && N > 0 && N % 4 == 0 && lds % 4 == 0 && ldp % 4 == 0, "lx_softmax_rows: N, lds, ldp must be multiples of 4");
  return softmax_launch<FmtBf16>("lx_softmax_rows", SoftmaxCall{S, lds, scale, P, ldp, 0, M, N, N, stream}, true);
}

extern "C" int lx_softmax_rows_valid(const float* S, int lds, float scale, void* P, int ldp, int M, int n_valid, int n_store, void* stream) {
  return softmax_run<FmtBf16>("lx_softmax_rows_valid", SoftmaxCall{S, lds, scale, P, ldp, 0, M, n_valid, n_store, stream}, false);
}

extern "C" int lx_softmax_rows_f16(const float* S, int lds, float scale, void* P, int ldp, int M, int n_valid, int n_store, void* stream) {
  return softmax_run<FmtF16>("lx_softmax_rows_f16", SoftmaxCall{S, lds, scale, P, ldp, 0, M, n_valid, n_store, stream}, true);
}

extern "C" int lx_softmax_rows_split(const float* S, int lds, float scale, void* P, int ldp, int p_lo_off, int M, int n_valid, int n_store, void* stream) {
  return softmax_run<FmtPair>("lx_softmax_rows_split", SoftmaxCall{S, lds, scale, P, ldp, p_lo_off, M, n_valid, n_store, stream}, false);
}

extern "C" int lx_convert_f16(void* dst, const void* src, int src_bf16, size_t n, int32_t* f16_ovf, void* stream) {
  LX_CHECK_ARG(dst && src, "lx_convert_f16: NULL operand");
  LX_CHECK_ARG(((uintptr_t)dst & 1) == 0 && ((uintptr_t)src & (src_bf16 ? 1 : 3)) == 0 && ((uintptr_t)f16_ovf & 3) == 0, "lx_convert_f16: misaligned operand");
  if (n == 0) return LX_OK;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(convert_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint16_t*)dst, src, src_bf16, n, (int*)f16_ovf);
  LX_LAUNCH_CHECK("lx_convert_f16");
  return LX_OK;
}
