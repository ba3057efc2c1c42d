// vae.hip -- row kernels of the FLUX VAE (diffusers AutoencoderKL; reference call sites src/flux/generate.py:375-380 decode,
// src/flux/pipeline_tools.py:7-30 encode) for gfx950. The VAE sits either side of the denoise loop; its
// convolutions run as implicit GEMMs on the DiT's MFMA kernel (lx_gemm_bf16: im2col rows x [Cout, 9 Cin] weights, fused
// bias / fp32 residual epilogues), so what lives here is the HBM-bound glue in NHWC layout:
//   * GroupNorm(32 groups, eps, affine) [+ SiLU]: partial sums per (image, row chunk, group), then one normalising pass;
//   * im2col for 3x3 convolutions: pad 1 / stride 1, the encoder's stride-2 downsample with its (0,1,0,1) padding, and the
//     decoder's nearest-neighbour 2x upsample folded into the gather (the upsampled image is never materialised);
//   * row softmax (fp32 scores -> bf16 probabilities) for the single-head mid-block attention, and its form for a key axis padded
//     to the GEMM's granule (token counts that are no multiple of 64): the pad keys get probability +0.
// GroupNorm and the padded softmax also store IEEE fp16 (the operand images of LX_OPERANDS_F16 launches: LxAutoencoderKL(operands="fp16")),
// from the same kernel bodies; with lx_convert_f16 they saturate at +-65504 and count the waves that clipped. im2col moves 16-bit words.
// All accesses are 8-16 B per lane along the channel axis (the padded softmax falls back to scalar ones on unaligned rows).
#include "common.h"

namespace {

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

template <typename T>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, int P, int C, int G, int rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[2][256];                         // every thread's (sum, sumsq); folded per group in a FIXED order (no atomics)
  const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
  const int lanes_per_row = C / 4, rows_per_iter = 256 / lanes_per_row;
  const int tid = threadIdx.x, c4 = (tid % lanes_per_row) * 4, rsub = tid / lanes_per_row;
  const int r0 = chunk * rows_per_chunk, r1 = min(P, r0 + rows_per_chunk);
  float s = 0.f, q = 0.f;                               // the thread's 4 channels lie in ONE group (C/G >= 4, multiple of 4)
  const T* xb = x + (size_t)b * P * C + c4;
  for (int r = r0 + rsub; r < r1; r += rows_per_iter) {
    const f32x4 v = load4<T>(xb + (size_t)r * C);
    s += (v[0] + v[1]) + (v[2] + v[3]);
    q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  red[0][tid] = s;
  red[1][tid] = q;
  __syncthreads();
  if (tid < G) {
    const int lpg = (C / G) / 4;                        // lanes per group within a row
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

// F16: y is the fp16 operand image of an LX_OPERANDS_F16 GEMM (round to nearest even, saturated to +-65504); a wave that clipped a value
// adds 1 to *f16_ovf (NULL: not reported). The bf16 instantiation never touches f16_ovf.
template <typename T, bool F16>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, int P, int C, int G, const float* __restrict__ part, int nchunk,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int silu,
                                                       uint16_t* __restrict__ y, int* __restrict__ f16_ovf) {
  const int b = blockIdx.y;
  float mx = 0.f;
  const size_t n4 = (size_t)P * C / 4;
  const float inv_n = 1.0f / ((float)P * (float)(C / G));
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int c4 = (int)((i * 4) % C);
    const int g = c4 / (C / G);
    float s = 0.f, q = 0.f;
    for (int k = 0; k < nchunk; ++k) {
      const float* p = part + (((size_t)b * nchunk + k) * G + g) * 2;
      s += p[0];
      q += p[1];
    }
    const float mean = s * inv_n;
    const float rstd = rsqrtf(fmaxf(q * inv_n - mean * mean, 0.f) + eps);
    const f32x4 v = load4<T>(x + (size_t)b * P * C + i * 4);
    const f32x4 ga = *(const f32x4*)(gamma + c4), be = *(const f32x4*)(beta + c4);
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t = (v[c] - mean) * rstd * ga[c] + be[c];
      if (silu) t = t / (1.0f + __expf(-t));
      o[c] = t;
    }
    *(u32x2*)(y + (size_t)b * P * C + i * 4) = u32x2{pack_op16x2<F16>(o[0], o[1], mx), pack_op16x2<F16>(o[2], o[3], mx)};
  }
  if constexpr (F16) report_f16_overflow(mx, f16_ovf);
}

// ---- im2col for 3x3 convolutions, NHWC bf16 -> [B*Ho*Wo, Kpad] bf16, column = (dy*3 + dx)*C + c ------------------------------------
// mode 0: stride 1, pad 1 (Ho = H, Wo = W);  mode 1: stride 2, pad (0,1,0,1) (Ho = H/2, Wo = W/2: diffusers Downsample2D with padding=0);
// mode 2: nearest 2x upsample, then stride 1 pad 1 (Ho = 2H, Wo = 2W: Upsample2D + its conv). Columns >= 9*C are zero padding.
__global__ __launch_bounds__(256) void im2col3x3_kernel(const uint16_t* __restrict__ x, int B, int H, int W, int C, int mode, uint16_t* __restrict__ out,
                                                        int Kpad) {
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  const int cv = C % 8 == 0 ? 8 : 1;                       // channels per work item
  const int per_tap = C / cv;
  const size_t items = (size_t)B * Ho * Wo * 9 * per_tap;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const int cc = (int)(i % per_tap) * cv;
    size_t r = i / per_tap;
    const int tap = (int)(r % 9);
    r /= 9;                                                // output pixel index (b, yo, xo)
    const int xo = (int)(r % Wo), yo = (int)((r / Wo) % Ho), b = (int)(r / ((size_t)Wo * Ho));
    const int dy = tap / 3, dx = tap % 3;
    int yi, xi;
    bool ok;
    if (mode == 1) { yi = 2 * yo + dy; xi = 2 * xo + dx; ok = yi < H && xi < W; }
    else if (mode == 2) { const int yu = yo + dy - 1, xu = xo + dx - 1; ok = yu >= 0 && yu < Ho && xu >= 0 && xu < Wo; yi = yu >> 1; xi = xu >> 1; }
    else { yi = yo + dy - 1; xi = xo + dx - 1; ok = yi >= 0 && yi < H && xi >= 0 && xi < W; }
    uint16_t* o = out + r * Kpad + tap * C + cc;
    const uint16_t* s = x + (((size_t)b * H + (ok ? yi : 0)) * W + (ok ? xi : 0)) * C + cc;
    if (cv == 8) *(u32x4*)o = ok ? *(const u32x4*)s : u32x4{0u, 0u, 0u, 0u};
    else *o = ok ? *s : (uint16_t)0;
  }
  // zero the K padding (columns [9C, Kpad))
  const int padc = Kpad - 9 * C;
  if (padc > 0) {
    const size_t rows = (size_t)B * Ho * Wo, n = rows * padc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[(i / padc) * Kpad + 9 * C + (i % padc)] = 0;
  }
}

// ---- row softmax: fp32 scores [M, N] (lds) * scale -> bf16 probabilities [M, N] (ldp). One wave per row. ----------------------------
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, int lds, float scale, uint16_t* __restrict__ Pm, int ldp, int M, int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* s = S + (size_t)row * lds;
  float m = -INFINITY;
  for (int c = lane * 4; c < N; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
    m = fmaxf(m, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  }
  m = wave_max(m) * scale;
  float l = 0.f;
  for (int c = lane * 4; c < N; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) l += __expf(v[k] * scale - m);
  }
  const float inv = 1.0f / wave_sum(l);
  uint16_t* p = Pm + (size_t)row * ldp;
  for (int c = lane * 4; c < N; c += 256) {
    const f32x4 v = *(const f32x4*)(s + c);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __expf(v[k] * scale - m) * inv;
    *(u32x2*)(p + c) = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
  }
}

// The 16-bit format of a probability image: how two / one fp32 values are stored. Probabilities are <= 1, so the fp16 form needs no
// saturation (and has no overflow to report).
struct StoreBf16 {
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
  static __device__ __forceinline__ uint16_t one(float v) { return f32_to_bf16(v); }
};
struct StoreF16 {
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    const f16x2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, v);
  }
  static __device__ __forceinline__ uint16_t one(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
};

// ---- row softmax over the first n_valid columns of a row whose key axis is padded: P[row, 0:n_valid] = softmax(scale * S[row, 0:n_valid]),
// P[row, n_valid:n_store] = +0. One wave per row. Columns >= n_valid of S (scores against padding: anything, NaN included) are never
// loaded; nothing at or beyond column n_store of P is written. VEC: every row of S starts 16-byte and every row of P 8-byte aligned, so
// columns [0, n_valid & ~3) go four per lane and only the < 4 columns behind them one per lane; otherwise every access is a scalar one.
template <bool VEC, typename ST>
__global__ __launch_bounds__(256) void softmax_rows_valid_kernel(const float* __restrict__ S, int lds, float scale, uint16_t* __restrict__ Pm, int ldp,
                                                                 int M, int n_valid, int n_store) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* s = S + (size_t)row * lds;
  uint16_t* p = Pm + (size_t)row * ldp;
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
    *(u32x2*)(p + c) = u32x2{ST::pack2(o[0], o[1]), ST::pack2(o[2], o[3])};
  }
  for (int c = nv + lane; c < n_valid; c += 64) p[c] = ST::one(__expf(s[c] * scale - m) * inv);
  // the pad keys' probabilities: scalar up to the next multiple of 4 (z0), vectors up to the last one (z1), scalar to n_store
  const int z0 = VEC ? min((n_valid + 3) & ~3, n_store) : n_store, z1 = VEC ? max(z0, n_store & ~3) : n_store;
  for (int c = n_valid + lane; c < z0; c += 64) p[c] = 0;
  for (int c = z0 + lane * 4; c < z1; c += 256) *(u32x2*)(p + c) = u32x2{0u, 0u};
  for (int c = z1 + lane; c < n_store; c += 64) p[c] = 0;
}

}  // namespace

extern "C" size_t lx_groupnorm_workspace_bytes(int B, int P, int G) {
  const int nchunk = P >= 4096 ? 64 : (P >= 256 ? 16 : 1);
  return (size_t)B * nchunk * G * 2 * sizeof(float);
}

// The two passes of lx_groupnorm_silu / lx_groupnorm_silu_f16 (arguments checked by the caller).
template <typename T, bool F16>
static void gn_launch(const T* x, int B, int P, int C, int G, const float* gamma, const float* beta, float eps, int silu, void* y, void* ws,
                      int32_t* f16_ovf, hipStream_t s) {
  const int nchunk = P >= 4096 ? 64 : (P >= 256 ? 16 : 1);
  const int rpc = (P + nchunk - 1) / nchunk;
  float* part = (float*)ws;
  const size_t n4 = (size_t)P * C / 4;
  const int gx = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(gn_stats_kernel<T>, dim3(nchunk, B), dim3(256), 0, s, x, P, C, G, rpc, part);
  hipLaunchKernelGGL((gn_apply_kernel<T, F16>), dim3(gx, B), dim3(256), 0, s, x, P, C, G, part, nchunk, gamma, beta, eps, silu, (uint16_t*)y, (int*)f16_ovf);
}

extern "C" int lx_groupnorm_silu(const void* x, int x_is_bf16, int B, int P, int C, int G, const float* gamma, const float* beta, float eps,
                                 int silu, void* y, void* ws, size_t ws_bytes, void* stream) {
  LX_CHECK_ARG(x && y && gamma && beta && ws, "lx_groupnorm_silu: NULL operand");
  LX_CHECK_ARG(B > 0 && P > 0 && C > 0 && G > 0 && G <= 64 && C % G == 0 && (C / G) % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "lx_groupnorm_silu: need G <= 64, C %% G == 0, (C/G) %% 4 == 0, C/4 a divisor of 256 (C=%d G=%d)", C, G);
  LX_CHECK_ARG(ws_bytes >= lx_groupnorm_workspace_bytes(B, P, G), "lx_groupnorm_silu: workspace too small");
  if (x_is_bf16) gn_launch<uint16_t, false>((const uint16_t*)x, B, P, C, G, gamma, beta, eps, silu, y, ws, nullptr, (hipStream_t)stream);
  else gn_launch<float, false>((const float*)x, B, P, C, G, gamma, beta, eps, silu, y, ws, nullptr, (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_groupnorm_silu");
  return LX_OK;
}

extern "C" int lx_groupnorm_silu_f16(const float* x, int B, int P, int C, int G, const float* gamma, const float* beta, float eps, int silu, void* y,
                                     void* ws, size_t ws_bytes, int32_t* f16_ovf, void* stream) {
  LX_CHECK_ARG(x && y && gamma && beta && ws, "lx_groupnorm_silu_f16: NULL operand");
  LX_CHECK_ARG(B > 0 && P > 0 && C > 0 && G > 0 && G <= 64 && C % G == 0 && (C / G) % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "lx_groupnorm_silu_f16: need G <= 64, C %% G == 0, (C/G) %% 4 == 0, C/4 a divisor of 256 (C=%d G=%d)", C, G);
  LX_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0 && ((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0 && ((uintptr_t)f16_ovf & 3) == 0, "lx_groupnorm_silu_f16: misaligned operand");
  LX_CHECK_ARG(ws_bytes >= lx_groupnorm_workspace_bytes(B, P, G), "lx_groupnorm_silu_f16: workspace too small");
  gn_launch<float, true>(x, B, P, C, G, gamma, beta, eps, silu, y, ws, f16_ovf, (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_groupnorm_silu_f16");
  return LX_OK;
}

extern "C" int lx_im2col3x3(const void* x, int B, int H, int W, int C, int mode, void* out, int Kpad, void* stream) {
  LX_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && C > 0, "lx_im2col3x3: bad arguments");
  LX_CHECK_ARG(mode >= 0 && mode <= 2 && (mode != 1 || (H % 2 == 0 && W % 2 == 0)), "lx_im2col3x3: mode 0|1|2 (mode 1 needs even H, W)");
  LX_CHECK_ARG(Kpad >= 9 * C && Kpad % 8 == 0, "lx_im2col3x3: Kpad=%d must be >= 9*C and a multiple of 8", Kpad);
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  const size_t items = (size_t)B * Ho * Wo * 9 * (C % 8 == 0 ? C / 8 : C);
  const int grid = (int)((items + 255) / 256 < 16384 ? (items + 255) / 256 : 16384);
  hipLaunchKernelGGL(im2col3x3_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, B, H, W, C, mode, (uint16_t*)out, Kpad);
  LX_LAUNCH_CHECK("lx_im2col3x3");
  return LX_OK;
}

extern "C" int lx_softmax_rows(const float* S, int lds, float scale, void* P, int ldp, int M, int N, void* stream) {
  LX_CHECK_ARG(S && P && M > 0 && N > 0 && N % 4 == 0 && lds % 4 == 0 && ldp % 4 == 0, "lx_softmax_rows: N, lds, ldp must be multiples of 4");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, M, N);
  LX_LAUNCH_CHECK("lx_softmax_rows");
  return LX_OK;
}

extern "C" int lx_softmax_rows_valid(const float* S, int lds, float scale, void* P, int ldp, int M, int n_valid, int n_store, void* stream) {
  LX_CHECK_ARG(S && P, "lx_softmax_rows_valid: NULL operand");
  LX_CHECK_ARG(M > 0 && n_valid >= 1 && n_store >= n_valid, "lx_softmax_rows_valid: need M > 0 and 1 <= n_valid <= n_store (M=%d n_valid=%d n_store=%d)", M, n_valid, n_store);
  LX_CHECK_ARG(lds >= n_valid && ldp >= n_store, "lx_softmax_rows_valid: need lds >= n_valid and ldp >= n_store (lds=%d ldp=%d n_valid=%d n_store=%d)", lds, ldp, n_valid, n_store);
  const bool vec = ((uintptr_t)S & 15) == 0 && lds % 4 == 0 && ((uintptr_t)P & 7) == 0 && ldp % 4 == 0;
  if (vec) hipLaunchKernelGGL((softmax_rows_valid_kernel<true, StoreBf16>), dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, M, n_valid, n_store);
  else hipLaunchKernelGGL((softmax_rows_valid_kernel<false, StoreBf16>), dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, M, n_valid, n_store);
  LX_LAUNCH_CHECK("lx_softmax_rows_valid");
  return LX_OK;
}

extern "C" int lx_softmax_rows_f16(const float* S, int lds, float scale, void* P, int ldp, int M, int n_valid, int n_store, void* stream) {
  LX_CHECK_ARG(S && P, "lx_softmax_rows_f16: NULL operand");
  LX_CHECK_ARG(M > 0 && n_valid >= 1 && n_store >= n_valid, "lx_softmax_rows_f16: need M > 0 and 1 <= n_valid <= n_store (M=%d n_valid=%d n_store=%d)", M, n_valid, n_store);
  LX_CHECK_ARG(lds >= n_valid && ldp >= n_store, "lx_softmax_rows_f16: need lds >= n_valid and ldp >= n_store (lds=%d ldp=%d n_valid=%d n_store=%d)", lds, ldp, n_valid, n_store);
  LX_CHECK_ARG(((uintptr_t)S & 3) == 0 && ((uintptr_t)P & 1) == 0, "lx_softmax_rows_f16: misaligned operand");
  const bool vec = ((uintptr_t)S & 15) == 0 && lds % 4 == 0 && ((uintptr_t)P & 7) == 0 && ldp % 4 == 0;
  if (vec) hipLaunchKernelGGL((softmax_rows_valid_kernel<true, StoreF16>), dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, M, n_valid, n_store);
  else hipLaunchKernelGGL((softmax_rows_valid_kernel<false, StoreF16>), dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, M, n_valid, n_store);
  LX_LAUNCH_CHECK("lx_softmax_rows_f16");
  return LX_OK;
}

// ---- fp32 | bf16 -> the fp16 operand image, saturated to +-65504 AND counted (lx_convert's dst 2 clips silently). NaN stays NaN.
namespace {
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
}  // namespace

extern "C" int lx_convert_f16(void* dst, const void* src, int src_bf16, size_t n, int32_t* f16_ovf, void* stream) {
  LX_CHECK_ARG(dst && src, "lx_convert_f16: NULL operand");
  LX_CHECK_ARG(((uintptr_t)dst & 1) == 0 && ((uintptr_t)src & (src_bf16 ? 1 : 3)) == 0 && ((uintptr_t)f16_ovf & 3) == 0, "lx_convert_f16: misaligned operand");
  if (n == 0) return LX_OK;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(convert_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (uint16_t*)dst, src, src_bf16, n, (int*)f16_ovf);
  LX_LAUNCH_CHECK("lx_convert_f16");
  return LX_OK;
}

// ==== precise mode: the same glue on split-bf16 operand pairs =======================================================================
// A pair image holds x as hi = bf16(x) at column c and lo = bf16(x - hi) at column lo_off + c of the same row (split_bf16_pair): the
// operand of a k_segs = 2 | 3 launch of lx_gemm_bf16. The residual stream between the GEMMs stays fp32.
namespace {

// ---- GroupNorm on fp32 x -> pair image. Same two passes and the same fixed-order fold as gn_stats_kernel / gn_apply_kernel, but the
// sums are taken of x - shift, shift = mean of the group's channels at pixel 0 of the image: a sample of the group, so |mean - shift| is
// of the order of the spread and E[d^2] - E[d]^2 cancels nothing to speak of, however large the mean is against the spread. The
// partials are fp32 (of the shifted values); they are combined, and the variance formed, in double.
__device__ __forceinline__ float gn_shift(const float* __restrict__ x0, int g, int cpg) {   // x0: pixel 0 of the image
  float s = 0.f;
  for (int j = 0; j < cpg; ++j) s += x0[g * cpg + j];
  return s / (float)cpg;
}

__global__ __launch_bounds__(256) void gn_stats_shift_kernel(const float* __restrict__ x, int P, int C, int G, int rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[2][256];
  const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
  const int lanes_per_row = C / 4, rows_per_iter = 256 / lanes_per_row;
  const int tid = threadIdx.x, c4 = (tid % lanes_per_row) * 4, rsub = tid / lanes_per_row;
  const int r0 = chunk * rows_per_chunk, r1 = min(P, r0 + rows_per_chunk);
  const int cpg = C / G;
  const float* x0 = x + (size_t)b * P * C;
  const float sh = gn_shift(x0, c4 / cpg, cpg);          // the thread's 4 channels lie in ONE group
  float s = 0.f, q = 0.f;
  const float* xb = x0 + c4;
  for (int r = r0 + rsub; r < r1; r += rows_per_iter) {
    f32x4 v = *(const f32x4*)(xb + (size_t)r * C);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] -= sh;
    s += (v[0] + v[1]) + (v[2] + v[3]);
    q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  red[0][tid] = s;
  red[1][tid] = q;
  __syncthreads();
  if (tid < G) {
    const int lpg = cpg / 4;
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

__global__ __launch_bounds__(256) void gn_apply_split_kernel(const float* __restrict__ x, int P, int C, int G, const float* __restrict__ part, int nchunk,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int silu,
                                                             uint16_t* __restrict__ y, int ldy, int y_lo_off) {
  const int b = blockIdx.y;
  const int cpg = C / G, c4s = C / 4;
  const size_t n4 = (size_t)P * c4s;
  const double inv_n = 1.0 / ((double)P * (double)cpg);
  const float* x0 = x + (size_t)b * P * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int c4 = (int)(i % c4s) * 4;
    const size_t p = i / c4s;
    const int g = c4 / cpg;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nchunk; ++k) {
      const float* pp = part + (((size_t)b * nchunk + k) * G + g) * 2;
      s += (double)pp[0];
      q += (double)pp[1];
    }
    const double md = s * inv_n;                          // mean - shift
    const float rstd = (float)(1.0 / sqrt(fmax(q * inv_n - md * md, 0.0) + (double)eps));
    const float mean = (float)((double)gn_shift(x0, g, cpg) + md);
    const f32x4 v = *(const f32x4*)(x0 + i * 4);
    const f32x4 ga = *(const f32x4*)(gamma + c4), be = *(const f32x4*)(beta + c4);
    uint16_t hh[4], ll[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float t = (v[c] - mean) * rstd * ga[c] + be[c];
      if (silu) t = t / (1.0f + __expf(-t));
      split_bf16_pair(t, hh[c], ll[c]);
    }
    uint16_t* o = y + ((size_t)b * P + p) * ldy + c4;
    *(u32x2*)o = u32x2{pack_u16x2(hh[0], hh[1]), pack_u16x2(hh[2], hh[3])};
    *(u32x2*)(o + y_lo_off) = u32x2{pack_u16x2(ll[0], ll[1]), pack_u16x2(ll[2], ll[3])};
  }
}

// ---- im2col3x3_kernel on a pair image: pixel rows [hi C | ... | lo C] (stride ldx, lo at x_lo_off) -> rows [hi taps Kpad | lo taps Kpad].
// A work item is (output pixel, half, tap, channel vector); the two halves are gathered independently, each exactly as the bf16 kernel does.
template <bool VEC>
__global__ __launch_bounds__(256) void im2col3x3_split_kernel(const uint16_t* __restrict__ x, int ldx, int x_lo_off, int B, int H, int W, int C, int mode,
                                                              uint16_t* __restrict__ out, int Kpad) {
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  constexpr int cv = VEC ? 8 : 1;
  const int per_tap = C / cv;
  const size_t rows = (size_t)B * Ho * Wo, items = rows * 18 * per_tap;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    const int cc = (int)(i % per_tap) * cv;
    size_t r = i / per_tap;
    const int tap = (int)(r % 9);
    r /= 9;
    const int half = (int)(r & 1);
    r >>= 1;                                               // output pixel index (b, yo, xo)
    const int xo = (int)(r % Wo), yo = (int)((r / Wo) % Ho), b = (int)(r / ((size_t)Wo * Ho));
    const int dy = tap / 3, dx = tap % 3;
    int yi, xi;
    bool ok;
    if (mode == 1) { yi = 2 * yo + dy; xi = 2 * xo + dx; ok = yi < H && xi < W; }
    else if (mode == 2) { const int yu = yo + dy - 1, xu = xo + dx - 1; ok = yu >= 0 && yu < Ho && xu >= 0 && xu < Wo; yi = yu >> 1; xi = xu >> 1; }
    else { yi = yo + dy - 1; xi = xo + dx - 1; ok = yi >= 0 && yi < H && xi >= 0 && xi < W; }
    uint16_t* o = out + r * (2 * (size_t)Kpad) + (size_t)half * Kpad + tap * C + cc;
    const uint16_t* s = x + (((size_t)b * H + (ok ? yi : 0)) * W + (ok ? xi : 0)) * ldx + half * x_lo_off + cc;
    if (VEC) *(u32x4*)o = ok ? *(const u32x4*)s : u32x4{0u, 0u, 0u, 0u};
    else *o = ok ? *s : (uint16_t)0;
  }
  // zero the K padding (columns [9C, Kpad) of both halves)
  const int padc = Kpad - 9 * C;
  if (padc > 0) {
    const size_t n = rows * 2 * padc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
      out[(i / padc) * Kpad + 9 * C + (i % padc)] = 0;      // i / padc = 2 * row + half, and a half is Kpad columns
  }
}

// ---- softmax_rows_valid_kernel with a pair output: hi at P[row, c], lo at P[row, p_lo_off + c]; +0 in [n_valid, n_store) of both halves.
// One wave per row; S is read as there (columns >= n_valid never). VEC additionally needs p_lo_off % 4 == 0.
template <bool VEC>
__global__ __launch_bounds__(256) void softmax_rows_split_kernel(const float* __restrict__ S, int lds, float scale, uint16_t* __restrict__ Pm, int ldp,
                                                                 int p_lo_off, int M, int n_valid, int n_store) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* s = S + (size_t)row * lds;
  uint16_t* p = Pm + (size_t)row * ldp;
  uint16_t* pl = p + p_lo_off;
  const int nv = VEC ? (n_valid & ~3) : 0;
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
    uint16_t hh[4], ll[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) split_bf16_pair(__expf(v[k] * scale - m) * inv, hh[k], ll[k]);
    *(u32x2*)(p + c) = u32x2{pack_u16x2(hh[0], hh[1]), pack_u16x2(hh[2], hh[3])};
    *(u32x2*)(pl + c) = u32x2{pack_u16x2(ll[0], ll[1]), pack_u16x2(ll[2], ll[3])};
  }
  for (int c = nv + lane; c < n_valid; c += 64) split_bf16_pair(__expf(s[c] * scale - m) * inv, p[c], pl[c]);
  const int z0 = VEC ? min((n_valid + 3) & ~3, n_store) : n_store, z1 = VEC ? max(z0, n_store & ~3) : n_store;
  for (int c = n_valid + lane; c < z0; c += 64) p[c] = pl[c] = 0;
  for (int c = z0 + lane * 4; c < z1; c += 256) *(u32x2*)(p + c) = *(u32x2*)(pl + c) = u32x2{0u, 0u};
  for (int c = z1 + lane; c < n_store; c += 64) p[c] = pl[c] = 0;
}

}  // namespace

extern "C" int lx_groupnorm_silu_split(const float* x, int B, int P, int C, int G, const float* gamma, const float* beta, float eps, int silu,
                                       void* y, int ldy, int y_lo_off, void* ws, size_t ws_bytes, void* stream) {
  LX_CHECK_ARG(x && y && gamma && beta && ws, "lx_groupnorm_silu_split: NULL operand");
  LX_CHECK_ARG(B > 0 && P > 0 && C > 0 && G > 0 && G <= 64 && C % G == 0 && (C / G) % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "lx_groupnorm_silu_split: need G <= 64, C %% G == 0, (C/G) %% 4 == 0, C/4 a divisor of 256 (C=%d G=%d)", C, G);
  LX_CHECK_ARG(y_lo_off % 8 == 0 && y_lo_off >= C && ldy % 4 == 0 && ldy >= y_lo_off + C, "lx_groupnorm_silu_split: need y_lo_off %% 8 == 0, C <= y_lo_off, y_lo_off + C <= ldy, ldy %% 4 == 0 (C=%d ldy=%d y_lo_off=%d)", C, ldy, y_lo_off);
  LX_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0 && ((uintptr_t)gamma & 15) == 0 && ((uintptr_t)beta & 15) == 0, "lx_groupnorm_silu_split: misaligned operand");
  LX_CHECK_ARG(ws_bytes >= lx_groupnorm_workspace_bytes(B, P, G), "lx_groupnorm_silu_split: workspace too small");
  const int nchunk = P >= 4096 ? 64 : (P >= 256 ? 16 : 1);
  const int rpc = (P + nchunk - 1) / nchunk;
  hipStream_t s = (hipStream_t)stream;
  const size_t n4 = (size_t)P * C / 4;
  const int gx = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(gn_stats_shift_kernel, dim3(nchunk, B), dim3(256), 0, s, x, P, C, G, rpc, (float*)ws);
  hipLaunchKernelGGL(gn_apply_split_kernel, dim3(gx, B), dim3(256), 0, s, x, P, C, G, (const float*)ws, nchunk, gamma, beta, eps, silu, (uint16_t*)y, ldy, y_lo_off);
  LX_LAUNCH_CHECK("lx_groupnorm_silu_split");
  return LX_OK;
}

extern "C" int lx_im2col3x3_split(const void* x, int ldx, int x_lo_off, int B, int H, int W, int C, int mode, void* out, int Kpad, void* stream) {
  LX_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && C > 0, "lx_im2col3x3_split: bad arguments");
  LX_CHECK_ARG(mode >= 0 && mode <= 2 && (mode != 1 || (H % 2 == 0 && W % 2 == 0)), "lx_im2col3x3_split: mode 0|1|2 (mode 1 needs even H, W)");
  LX_CHECK_ARG(Kpad >= 9 * C && Kpad % 8 == 0, "lx_im2col3x3_split: Kpad=%d must be >= 9*C and a multiple of 8", Kpad);
  LX_CHECK_ARG(x_lo_off % 8 == 0 && x_lo_off >= C && ldx >= x_lo_off + C, "lx_im2col3x3_split: need x_lo_off %% 8 == 0 and C <= x_lo_off, x_lo_off + C <= ldx (C=%d ldx=%d x_lo_off=%d)", C, ldx, x_lo_off);
  const int Ho = mode == 1 ? H / 2 : (mode == 2 ? 2 * H : H), Wo = mode == 1 ? W / 2 : (mode == 2 ? 2 * W : W);
  const bool vec = C % 8 == 0 && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const size_t items = (size_t)B * Ho * Wo * 18 * (vec ? C / 8 : C);
  const int grid = (int)((items + 255) / 256 < 16384 ? (items + 255) / 256 : 16384);
  if (vec) hipLaunchKernelGGL(im2col3x3_split_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, x_lo_off, B, H, W, C, mode, (uint16_t*)out, Kpad);
  else hipLaunchKernelGGL(im2col3x3_split_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, x_lo_off, B, H, W, C, mode, (uint16_t*)out, Kpad);
  LX_LAUNCH_CHECK("lx_im2col3x3_split");
  return LX_OK;
}

extern "C" int lx_softmax_rows_split(const float* S, int lds, float scale, void* P, int ldp, int p_lo_off, int M, int n_valid, int n_store, void* stream) {
  LX_CHECK_ARG(S && P, "lx_softmax_rows_split: NULL operand");
  LX_CHECK_ARG(M > 0 && n_valid >= 1 && n_store >= n_valid, "lx_softmax_rows_split: need M > 0 and 1 <= n_valid <= n_store (M=%d n_valid=%d n_store=%d)", M, n_valid, n_store);
  LX_CHECK_ARG(lds >= n_valid && p_lo_off % 8 == 0 && p_lo_off >= n_store && ldp >= p_lo_off + n_store, "lx_softmax_rows_split: need lds >= n_valid, p_lo_off %% 8 == 0 and n_store <= p_lo_off, p_lo_off + n_store <= ldp (lds=%d ldp=%d p_lo_off=%d n_valid=%d n_store=%d)", lds, ldp, p_lo_off, n_valid, n_store);
  const bool vec = ((uintptr_t)S & 15) == 0 && lds % 4 == 0 && ((uintptr_t)P & 7) == 0 && ldp % 4 == 0;
  if (vec) hipLaunchKernelGGL(softmax_rows_split_kernel<true>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, p_lo_off, M, n_valid, n_store);
  else hipLaunchKernelGGL(softmax_rows_split_kernel<false>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lds, scale, (uint16_t*)P, ldp, p_lo_off, M, n_valid, n_store);
  LX_LAUNCH_CHECK("lx_softmax_rows_split");
  return LX_OK;
}
