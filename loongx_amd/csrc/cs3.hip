// cs3.hip -- CS3 (Cross-Scale State Space) encoder kernels for gfx950. fp32 I/O, channel-major [B,C,L].
//
// Reference: src/train/model.py EEGEncoder :16-134, PPG :137-205, fNIRS :208-274, Motion :277-343,
// FeaturePyramidPooling :345-373 (+ s4torch.S4Model, restated in oracle/s4.py).
//
// The S4 layer is an LTI state-space model.  s4torch evaluates it as an FFT convolution with the length-L
// kernel K[h,l]; here the same operator runs as a linear recurrence in modal form,
//     y[l] = Re sum_n w_n s_n[l] + D u[l],   s_n[l] = lam_n s_n[l-1] + u[l],
// evaluated by a WAVEFRONT PREFIX SCAN: the 64 lanes of a wave each own L/64 consecutive time steps of one
// (batch, channel) sequence (read with coalesced loads and handed to the lanes through LDS: seq_to_lanes), run the recurrence locally, exchange chunk carries with a 6-step Kogge-Stone
// scan over the wave (multiplier lam^(L/64), squared each step), and replay with the carry-in.  HiPPO-LegS
// modes cancel by up to ~1e10 at n=64 (oracle/s4.py::diagonalize), so the state and the output accumulator
// are fp64 -- MI355X runs vector fp64 at half the fp32 rate, and the op is tiny next to the DiT.
// lx_s4_conv is the same operator as a direct causal convolution with the materialised kernel (cross-check).
#include "common.h"

namespace {

// A sequence's samples reach the lanes through LDS: the workgroup reads its NT * CH consecutive floats with lane-CONTIGUOUS loads (one
// 256-B run per wave and instruction; 16 B per lane when CH % 4 == 0), and every lane then takes the CH consecutive samples it owns from
// LDS (rows of CH + 1 floats: conflict-free). Until round 5 a lane loaded its own chunk straight from HBM -- 16 B per lane at a CH * 4-byte
// stride, i.e. 64 different 256-B-apart addresses per load instruction. Results are the same bits; the output goes back the same way.
template <int CH, int NT>
__device__ __forceinline__ void seq_to_lanes(const float* __restrict__ src, float* __restrict__ lds, float (&uf)[CH], int tid) {
  if constexpr (CH % 4 == 0) {
#pragma unroll
    for (int it = 0; it < CH / 4; ++it) {
      const int i = (it * NT + tid) * 4;               // float index in the sequence: lanes on consecutive 16-byte pieces
      const f32x4 v = *(const f32x4*)(src + i);
      float* d = lds + (i / CH) * (CH + 1) + (i % CH);
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  } else {
#pragma unroll
    for (int it = 0; it < CH; ++it) {
      const int i = it * NT + tid;
      lds[(i / CH) * (CH + 1) + (i % CH)] = src[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CH; ++j) uf[j] = lds[tid * (CH + 1) + j];
  __syncthreads();
}
template <int CH, int NT>
__device__ __forceinline__ void lanes_to_seq(float* __restrict__ dst, float* __restrict__ lds, const float (&yf)[CH], int tid) {
#pragma unroll
  for (int j = 0; j < CH; ++j) lds[tid * (CH + 1) + j] = yf[j];
  __syncthreads();
  if constexpr (CH % 4 == 0) {
#pragma unroll
    for (int it = 0; it < CH / 4; ++it) {
      const int i = (it * NT + tid) * 4;
      const float* d = lds + (i / CH) * (CH + 1) + (i % CH);
      *(f32x4*)(dst + i) = f32x4{d[0], d[1], d[2], d[3]};
    }
  } else {
#pragma unroll
    for (int it = 0; it < CH; ++it) {
      const int i = it * NT + tid;
      dst[i] = lds[(i / CH) * (CH + 1) + (i % CH)];
    }
  }
}

template <int CH>
__global__ __launch_bounds__(64) void s4_scan_kernel(const float* __restrict__ u, const double* __restrict__ lam,
                                                     const double* __restrict__ w, const float* __restrict__ Dskip,
                                                     float* __restrict__ y, int H, int L, int N) {
  __shared__ float stage[64 * (CH + 1)];
  const int bh = blockIdx.x;
  const int h = bh % H;
  const int lane = threadIdx.x;
  float uf[CH];
  seq_to_lanes<CH, 64>(u + (size_t)bh * L, stage, uf, lane);
  double yacc[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) yacc[j] = 0.0;

  for (int n = 0; n < N; ++n) {
    const double lr = lam[((size_t)h * N + n) * 2], li = lam[((size_t)h * N + n) * 2 + 1];
    const double wr = w[((size_t)h * N + n) * 2], wi = w[((size_t)h * N + n) * 2 + 1];
    // pass A: chunk end state from a zero start, and lam^CH
    double er = 0.0, ei = 0.0, qr = 1.0, qi = 0.0;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const double tr = lr * er - li * ei + (double)uf[j];
      ei = lr * ei + li * er;
      er = tr;
      const double t2 = qr * lr - qi * li;
      qi = qr * li + qi * lr;
      qr = t2;
    }
    // Kogge-Stone inclusive scan of X_i = e_i + lam^CH * X_{i-1} across the 64 lanes
    double xr = er, xi = ei;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double sr = __shfl_up(xr, d, 64), si = __shfl_up(xi, d, 64);
      if (lane >= d) {
        xr += qr * sr - qi * si;
        xi += qr * si + qi * sr;
      }
      const double t2 = qr * qr - qi * qi;
      qi = 2.0 * qr * qi;
      qr = t2;
    }
    double sr = __shfl_up(xr, 1, 64), si = __shfl_up(xi, 1, 64);
    if (lane == 0) { sr = 0.0; si = 0.0; }
    // pass B: replay with the carry-in, accumulate Re(w * s)
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const double tr = lr * sr - li * si + (double)uf[j];
      si = lr * si + li * sr;
      sr = tr;
      yacc[j] += wr * sr - wi * si;
    }
  }
  const double dk = (double)Dskip[h];
  float yf[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) yf[j] = (float)(yacc[j] + dk * (double)uf[j]);
  lanes_to_seq<CH, 64>(y + (size_t)bh * L, stage, yf, lane);
}

// The same scan with NW waves per sequence (block = NW x 64 lanes, lane g owns time steps [g*CH, (g+1)*CH)): a [B, H] = [1, 64]
// layer is 64 one-wave blocks on a 256-CU part with the kernel above; four waves per sequence put a wave on every CU and
// shorten each lane's serial recurrence 4x. Wave totals travel through LDS (double-buffered: one barrier per mode), the carry
// into wave w is the NW-term recurrence C_w = T_{w-1} + lam^(64 CH) C_{w-1}, and lane i adds lam^(CH i) C_w to its in-wave
// prefix -- the powers fall out of the Kogge-Stone squaring chain.
template <int CH, int NW>
__global__ __launch_bounds__(64 * NW) void s4_scan_mw_kernel(const float* __restrict__ u, const double* __restrict__ lam,
                                                           const double* __restrict__ w, const float* __restrict__ Dskip,
                                                           float* __restrict__ y, int H, int L, int N) {
  __shared__ double tot[2][NW][2];
  __shared__ float stage[64 * NW * (CH + 1)];
  const int bh = blockIdx.x, h = bh % H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = wave * 64 + lane;
  float uf[CH];
  seq_to_lanes<CH, 64 * NW>(u + (size_t)bh * L, stage, uf, g);
  double yacc[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) yacc[j] = 0.0;
  for (int n = 0; n < N; ++n) {
    const double lr = lam[((size_t)h * N + n) * 2], li = lam[((size_t)h * N + n) * 2 + 1];
    const double wr = w[((size_t)h * N + n) * 2], wi = w[((size_t)h * N + n) * 2 + 1];
    double er = 0.0, ei = 0.0, qr = 1.0, qi = 0.0;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const double tr = lr * er - li * ei + (double)uf[j];
      ei = lr * ei + li * er;
      er = tr;
      const double t2 = qr * lr - qi * li;
      qi = qr * li + qi * lr;
      qr = t2;
    }
    double xr = er, xi = ei, pr = 1.0, pi = 0.0;         // p = (lam^CH)^lane, built from the squaring chain
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double sr = __shfl_up(xr, d, 64), si = __shfl_up(xi, d, 64);
      if (lane >= d) {
        xr += qr * sr - qi * si;
        xi += qr * si + qi * sr;
      }
      if (lane & d) {
        const double t = pr * qr - pi * qi;
        pi = pr * qi + pi * qr;
        pr = t;
      }
      const double t2 = qr * qr - qi * qi;
      qi = 2.0 * qr * qi;
      qr = t2;
    }                                                     // now q = lam^(64 CH)
    if (lane == 63) { tot[n & 1][wave][0] = xr; tot[n & 1][wave][1] = xi; }
    __syncthreads();
    double cr = 0.0, ci = 0.0;                            // carry into this wave
#pragma unroll
    for (int v = 0; v < NW - 1; ++v)
      if (v < wave) {
        const double t = qr * cr - qi * ci + tot[n & 1][v][0];
        ci = qr * ci + qi * cr + tot[n & 1][v][1];
        cr = t;
      }
    double sr = __shfl_up(xr, 1, 64), si = __shfl_up(xi, 1, 64);
    if (lane == 0) { sr = 0.0; si = 0.0; }
    sr += pr * cr - pi * ci;
    si += pr * ci + pi * cr;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const double tr = lr * sr - li * si + (double)uf[j];
      si = lr * si + li * sr;
      sr = tr;
      yacc[j] += wr * sr - wi * si;
    }
  }
  const double dk = (double)Dskip[h];
  float yf[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) yf[j] = (float)(yacc[j] + dk * (double)uf[j]);
  lanes_to_seq<CH, 64 * NW>(y + (size_t)bh * L, stage, yf, g);
}

// direct causal convolution: block per (b,h); K and u staged in LDS
__global__ __launch_bounds__(256) void s4_conv_kernel(const float* __restrict__ u, const float* __restrict__ Kk,
                                                      const float* __restrict__ Dskip, float* __restrict__ y, int H, int L) {
  extern __shared__ float sm[];
  float* ks = sm;
  float* us = sm + L;
  const int bh = blockIdx.x, h = bh % H;
  for (int i = threadIdx.x; i < L; i += 256) {
    ks[i] = Kk[(size_t)h * L + i];
    us[i] = u[(size_t)bh * L + i];
  }
  __syncthreads();
  const float dk = Dskip[h];
  for (int l = threadIdx.x; l < L; l += 256) {
    float a0 = 0.f, a1 = 0.f;
    int j = 0;
    for (; j + 1 <= l; j += 2) {
      a0 = fmaf(ks[j], us[l - j], a0);
      a1 = fmaf(ks[j + 1], us[l - j - 1], a1);
    }
    if (j <= l) a0 = fmaf(ks[j], us[l - j], a0);
    y[(size_t)bh * L + l] = a0 + a1 + dk * us[l];
  }
}

// pointwise channel mix (+GELU in, +residual, +LayerNorm over channels); thread = one (b, l) position
template <int HIN, int HOUT>
__global__ __launch_bounds__(256) void chanmix_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                      const float* __restrict__ bias, const float* __restrict__ resid,
                                                      const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                      float* __restrict__ y, int L, int act) {
  __shared__ float ws[HOUT * HIN + HOUT];
  for (int i = threadIdx.x; i < HOUT * HIN; i += 256) ws[i] = W[i];
  for (int i = threadIdx.x; i < HOUT; i += 256) ws[HOUT * HIN + i] = bias ? bias[i] : 0.f;
  __syncthreads();
  const int b = blockIdx.y;
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l >= L) return;
  float xin[HIN];
#pragma unroll
  for (int i = 0; i < HIN; ++i) {
    float v = x[((size_t)b * HIN + i) * L + l];
    if (act == 1) v = 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
    xin[i] = v;
  }
  float out[HOUT];
#pragma unroll
  for (int o = 0; o < HOUT; ++o) {
    float a = ws[HOUT * HIN + o];
#pragma unroll
    for (int i = 0; i < HIN; ++i) a = fmaf(ws[o * HIN + i], xin[i], a);
    if (resid) a += resid[((size_t)b * HOUT + o) * L + l];
    out[o] = a;
  }
  if (ln_g) {
    float m = 0.f;
#pragma unroll
    for (int o = 0; o < HOUT; ++o) m += out[o];
    m /= (float)HOUT;
    float v = 0.f;
#pragma unroll
    for (int o = 0; o < HOUT; ++o) v += (out[o] - m) * (out[o] - m);
    const float r = rsqrtf(v / (float)HOUT + 1e-5f);
#pragma unroll
    for (int o = 0; o < HOUT; ++o) out[o] = (out[o] - m) * r * ln_g[o] + ln_b[o];
  }
#pragma unroll
  for (int o = 0; o < HOUT; ++o) y[((size_t)b * HOUT + o) * L + l] = out[o];
}

struct PoolSizes { int n; int size[8]; int off[9]; };

__global__ void pyramid_pool_kernel(const float* __restrict__ x, float* __restrict__ y, int BC, int L, PoolSizes ps, int ldy, int y_col0) {
  const int total = ps.off[ps.n];
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)BC * total) return;
  const int row = (int)(idx / total), col = (int)(idx % total);
  int lvl = 0;
  for (int i = 1; i < ps.n; ++i)
    if (col >= ps.off[i]) lvl = i;
  const int j = col - ps.off[lvl], s = ps.size[lvl];
  const int st = (int)(((long)j * L) / s);
  const int en = (int)((((long)(j + 1)) * L + s - 1) / s);
  const float* xr = x + (size_t)row * L;
  float a = 0.f;
  for (int i = st; i < en; ++i) a += xr[i];
  y[(size_t)row * ldy + y_col0 + col] = a / (float)(en - st);
}

// Statistics are taken of x - x[0]: a row that sits on a large offset (mean 1e3, deviations of a few units) would otherwise lose the
// fp32 rounding of its MEAN (half an ulp of 1e3 = 3e-5) in every x - mean, 2e-5 of the output; the differences from the row's first
// element are small and (nearly) exact, and LayerNorm does not depend on the shift.
__global__ __launch_bounds__(256) void layernorm_relu_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ bta, int D, float eps) {
  __shared__ float red[8];
  float* xr = x + (size_t)blockIdx.x * D;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float piv = xr[0];
  float s = 0.f;
  for (int i = tid; i < D; i += 256) s += xr[i] - piv;
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)D;      // of x - piv
  float q = 0.f;
  for (int i = tid; i < D; i += 256) { const float d = (xr[i] - piv) - mean; q += d * d; }
  q = wave_sum(q);
  if (lane == 0) red[4 + wave] = q;
  __syncthreads();                                                         // (every thread has read xr[0] before anyone overwrites it)
  const float rstd = rsqrtf((red[4] + red[5] + red[6] + red[7]) / (float)D + eps);
  for (int i = tid; i < D; i += 256) {
    const float v = ((xr[i] - piv) - mean) * rstd * g[i] + bta[i];
    xr[i] = v > 0.f ? v : 0.f;
  }
}

// fp32 tiled GEMM Y[M,N] (=|+=) X[M,K] W[N,K]^T + bias; 64x64 tile, BK=16, 4x4 outputs per thread.
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ X, int ldx, int x_trans, const float* __restrict__ W,
                                                         int ldw, const float* __restrict__ bias, float* __restrict__ Y, int ldy,
                                                         int y_trans, int M, int N, int K, int accumulate) {
  __shared__ float xs[16][64 + 4];
  __shared__ float wsm[16][64 + 4];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int tm = (tid >> 4) * 4, tn = (tid & 15) * 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    // 64x16 tile of each operand: 1024 elements, 4 per thread
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + e * 256;
      int r, kk;
      if (x_trans) { kk = idx >> 6; r = idx & 63; } else { r = idx >> 4; kk = idx & 15; }
      float v = 0.f;
      if (m0 + r < M && k0 + kk < K) v = x_trans ? X[(size_t)(k0 + kk) * ldx + m0 + r] : X[(size_t)(m0 + r) * ldx + k0 + kk];
      xs[kk][r] = v;
      const int rw = idx >> 4, kw = idx & 15;
      float wv = 0.f;
      if (n0 + rw < N && k0 + kw < K) wv = W[(size_t)(n0 + rw) * ldw + k0 + kw];
      wsm[kw][rw] = wv;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const f32x4 a = *(const f32x4*)&xs[kk][tm];
      const f32x4 b = *(const f32x4*)&wsm[kk][tn];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + tm + i, n = n0 + tn + j;
      if (m < M && n < N) {
        float v = acc[i][j] + (bias ? bias[n] : 0.f);
        float* yp = y_trans ? (Y + (size_t)n * ldy + m) : (Y + (size_t)m * ldy + n);
        *yp = accumulate ? (*yp + v) : v;
      }
    }
}

// fp32 linear for a FEW rows (M <= 16: the encoder projection heads, 16384 -> 2048 -> 4096 ...): weight streaming, HBM bound.
// A wave owns 2 output columns and streams their weight rows once with 16-B loads (lanes split K); the M x-rows of each
// 256-wide K chunk are staged ONCE per block in LDS and shared by its 4 waves (reading x per wave from L2 made the kernel
// L2-bound: 16 x loads per 2 weight loads), all rows' accumulators stay in registers; N/8 blocks: a 16384 x 2048 layer puts one
// block on every CU. No split-K, no atomics: each output is one wave's shuffle reduction in a fixed order.
template <int MR>
__global__ __launch_bounds__(256) void linear_f32_skinny_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                                                const float* __restrict__ bias, float* __restrict__ Y, int ldy, int M, int N,
                                                                int K, int accumulate) {
  __shared__ __attribute__((aligned(16))) float xs[2][MR][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = (blockIdx.x * 4 + wave) * 2;
  const bool active = n0 < N;
  const float* w0 = W + (size_t)min(n0, N - 1) * ldw;
  const float* w1 = W + (size_t)min(n0 + 1, N - 1) * ldw;
  float acc[MR][2];
#pragma unroll
  for (int i = 0; i < MR; ++i) acc[i][0] = acc[i][1] = 0.f;
  auto stage = [&](int k0, int buf) {           // MR x 256 floats: thread -> (row = tid / 64 + 4 j, 4 consecutive k)
#pragma unroll
    for (int j = 0; j < (MR + 3) / 4; ++j) {
      const int r = (tid >> 6) + 4 * j, k = k0 + (tid & 63) * 4;
      if (r < MR) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < M && k < K) v = *(const f32x4*)(X + (size_t)r * ldx + k);
        *(f32x4*)&xs[buf][r][(tid & 63) * 4] = v;
      }
    }
  };
  stage(0, 0);
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += 256, buf ^= 1) {
    __syncthreads();                              // chunk k0 is in xs[buf]; everyone is done with xs[buf ^ 1]
    if (k0 + 256 < K) stage(k0 + 256, buf ^ 1);
    const int k = k0 + lane * 4;
    if (active && k < K) {
      const f32x4 a = *(const f32x4*)(w0 + k), b = *(const f32x4*)(w1 + k);
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        const f32x4 x = *(const f32x4*)&xs[buf][i][lane * 4];
        acc[i][0] = fmaf(x[0], a[0], fmaf(x[1], a[1], fmaf(x[2], a[2], fmaf(x[3], a[3], acc[i][0]))));
        acc[i][1] = fmaf(x[0], b[0], fmaf(x[1], b[1], fmaf(x[2], b[2], fmaf(x[3], b[3], acc[i][1]))));
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float v = wave_sum(acc[i][c]);
      if (lane == 0 && i < M && n0 + c < N) {
        float* yp = Y + (size_t)i * ldy + n0 + c;
        const float o = v + (bias ? bias[n0 + c] : 0.f);
        *yp = accumulate ? (*yp + o) : o;
      }
    }
}

// ---- channel-major fp32 GEMM on the f32-input MFMA:  Y[b][n][l] = epi(sum_k W[n][k] * X[b][k][l] + bias[n]) ---------------------------
// The CS3 / DGF side keeps activations channel-major [B, C, L]; a Linear over channels at every position (fuse_eeg's
// Linear(1024 -> 512), the two 1x1 convolutions of the DUAN gate) is W . X with X's positions along the fast axis -- exactly
// the B operand of v_mfma_f32_32x32x2_f32 (lane = position, k = channel), so no transpose is needed and the products are exact
// fp32. Block = 4 waves = a 64 (n) x 64 (l) tile, K in chunks of 32 staged through LDS (W rows padded to 33 floats:
// conflict-free column reads). Epilogues: 0 store, 1 accumulate into Y, 2 ReLU, 3 sigmoid + sum over the tile's 64 positions
// (-> part[b][l_tile][n], the DUAN gate's mean over L, summed later in tile order: no atomics).
constexpr int CG_KC = 32;
__global__ __launch_bounds__(256) void chan_gemm_f32_kernel(const float* __restrict__ X, long x_bstride, int ldx, const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias, float* __restrict__ Y, long y_bstride, int ldy,
                                                            int N, int K, int L, int epi, float* __restrict__ part) {
  __shared__ float Ws[64 * (CG_KC + 1)];
  __shared__ __attribute__((aligned(16))) float Xs[CG_KC * 64];
  const int b = blockIdx.z, n0 = blockIdx.y * 64, l0 = blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wn = wave >> 1, wl = wave & 1;
  const float* Xb = X + (size_t)b * x_bstride;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += CG_KC) {
    __syncthreads();
    // W tile [64 n][32 k]: thread -> (n = tid / 4 (+ 0), 8 consecutive k)
    {
      const int n = tid >> 2, kq = (tid & 3) * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n0 + n < N && k0 + kq + 4 * h < K) v = *(const f32x4*)(W + (size_t)(n0 + n) * ldw + k0 + kq + 4 * h);
#pragma unroll
        for (int c = 0; c < 4; ++c) Ws[n * (CG_KC + 1) + kq + 4 * h + c] = v[c];
      }
      // X tile [32 k][64 l]: thread -> (k = tid / 8, 8 consecutive l)
      const int k = tid >> 3, lq = (tid & 7) * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int l = l0 + lq + 4 * h;
        if (k0 + k < K && l + 3 < L) v = *(const f32x4*)(Xb + (size_t)(k0 + k) * ldx + l);
        else if (k0 + k < K) {
#pragma unroll
          for (int c = 0; c < 4; ++c) if (l + c < L) v[c] = Xb[(size_t)(k0 + k) * ldx + l + c];
        }
        *(f32x4*)&Xs[k * 64 + lq + 4 * h] = v;
      }
    }
    __syncthreads();
    const float* ap = Ws + (wn * 32 + l31) * (CG_KC + 1) + hi;
    const float* bp = Xs + hi * 64 + wl * 32 + l31;
#pragma unroll
    for (int st = 0; st < CG_KC / 2; ++st) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * st], bp[2 * st * 64], acc, 0, 0, 0);
  }
  // acc[r]: n = n0 + wn*32 + 8*(r/4) + 4*hi + r%4 ; l = l0 + wl*32 + l31
  const int l = l0 + wl * 32 + l31;
  float* Yb = Y ? Y + (size_t)b * y_bstride : nullptr;
  if (epi == 3) {
    __syncthreads();                                   // Xs is free: 64 n x 2 halves of partial sums
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int nl = wn * 32 + 8 * (r >> 2) + 4 * hi + (r & 3), n = n0 + nl;
      float v = 0.f;
      if (n < N && l < L) v = 1.0f / (1.0f + __expf(-(acc[r] + (bias ? bias[n] : 0.f))));
      // sum over the 32 positions of this wave's half tile: lanes of one half-wave (same hi) hold the same n
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (l31 == 0) Xs[nl * 2 + wl] = v;
    }
    __syncthreads();
    if (tid < 64 && n0 + tid < N) part[((size_t)b * gridDim.x + blockIdx.x) * N + n0 + tid] = Xs[tid * 2] + Xs[tid * 2 + 1];
    return;
  }
  if (l >= L) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wn * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
    if (n >= N) continue;
    float v = acc[r] + (bias ? bias[n] : 0.f);
    float* yp = Yb + (size_t)n * ldy + l;
    if (epi == 1) v += *yp;
    else if (epi == 2) v = v > 0.f ? v : 0.f;
    *yp = v;
  }
}

// ---- the same operator on the bf16 matrix pipe, fp32-class: Y = epi(W . X + bias) with every operand a bf16 PAIR -------------------
// x = x_hi + x_lo (x_hi = bf16(x), x_lo = bf16(x - x_hi): 16 significand bits), W likewise, and W . X evaluated as W_hi X_lo + W_lo X_hi +
// W_hi X_hi on v_mfma_f32_32x32x16_bf16 into one fp32 accumulation (the dropped W_lo X_lo term is 2^-18 relative): three MFMAs of 16-deep k
// where the exact-fp32 form needs eight of 2-deep k -- 16 / 3 of its rate (precise.hip's trick). The DUAN gate's two 1x1
// convolutions are 17.2 GFLOP of this per batch-16 call and were the reason `duan_norm_prompt` ran at 0.8 TB/s of its algorithmic bytes
// (fp32-matrix-bound at 157 TFLOP/s peak, not HBM-bound: round 4). Layout: a 64 (n) x 64 (l) tile per 4 waves as above, K in chunks of 64;
// the split happens ONCE per element at staging time -- W rows as they are, X transposed on the way into LDS (thread = one position l,
// 16 channels k: lane-contiguous 4-byte global loads, then 16 consecutive k of its l as two 16-byte LDS stores per image) so that both
// MFMA operands are one ds_read_b128 per lane (rows of 72 bf16 = 144 B: the 16 lanes of a read phase hit 64 distinct banks).
constexpr int CS_KC = 64, CS_LD = 72;
__global__ __launch_bounds__(256) void chan_gemm_split_kernel(const float* __restrict__ X, long x_bstride, int ldx, const float* __restrict__ W, int ldw,
                                                              const float* __restrict__ bias, float* __restrict__ Y, long y_bstride, int ldy,
                                                              int N, int K, int L, int epi, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint16_t Wh[64 * CS_LD], Wl[64 * CS_LD], Xh[64 * CS_LD], Xl[64 * CS_LD];
  const int b = blockIdx.z, n0 = blockIdx.y * 64, l0 = blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wn = wave >> 1, wl = wave & 1;
  const float* Xb = X + (size_t)b * x_bstride;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // staging roles: W: thread -> (row n = tid / 4, 16 consecutive k); X: thread -> (position l = tid % 64, 16 consecutive k)
  const int wn_s = tid >> 2, wk_s = (tid & 3) * 16;
  const int xl_s = tid & 63, xk_s = (tid >> 6) * 16;
  const bool w_ok = n0 + wn_s < N, x_ok = l0 + xl_s < L;
  float wr[16], xr[16];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (w_ok && k0 + wk_s + 4 * q < K) v = *(const f32x4*)(W + (size_t)(n0 + wn_s) * ldw + k0 + wk_s + 4 * q);     // (K % 4 == 0)
#pragma unroll
      for (int c = 0; c < 4; ++c) wr[4 * q + c] = v[c];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) xr[j] = (x_ok && k0 + xk_s + j < K) ? Xb[(size_t)(k0 + xk_s + j) * ldx + l0 + xl_s] : 0.f;
  };
  auto split_store = [&](const float (&v)[16], uint16_t* dh, uint16_t* dl) {
    u32x4 h[2], l[2];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint16_t a = f32_to_bf16(v[2 * q]), c = f32_to_bf16(v[2 * q + 1]);
      h[q >> 2][q & 3] = (uint32_t)a | ((uint32_t)c << 16);
      l[q >> 2][q & 3] = pack_bf16x2(v[2 * q] - bf16_to_f32(a), v[2 * q + 1] - bf16_to_f32(c));
    }
    *(u32x4*)dh = h[0]; *(u32x4*)(dh + 8) = h[1];
    *(u32x4*)dl = l[0]; *(u32x4*)(dl + 8) = l[1];
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += CS_KC) {
    __syncthreads();                                   // the previous chunk's fragments have been read
    split_store(wr, Wh + wn_s * CS_LD + wk_s, Wl + wn_s * CS_LD + wk_s);
    split_store(xr, Xh + xl_s * CS_LD + xk_s, Xl + xl_s * CS_LD + xk_s);
    __syncthreads();
    if (k0 + CS_KC < K) fetch(k0 + CS_KC);             // the next chunk's loads fly under this chunk's MFMAs
    const int ao = (wn * 32 + l31) * CS_LD + hi * 8, bo = (wl * 32 + l31) * CS_LD + hi * 8;
#pragma unroll
    for (int ks = 0; ks < CS_KC / 16; ++ks) {
      const bf16x8 ah = *(const bf16x8*)(Wh + ao + ks * 16), al = *(const bf16x8*)(Wl + ao + ks * 16);
      const bf16x8 bh = *(const bf16x8*)(Xh + bo + ks * 16), bl = *(const bf16x8*)(Xl + bo + ks * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);       // small terms first
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    }
  }
  // acc[r]: n = n0 + wn*32 + 8*(r/4) + 4*hi + r%4 ; l = l0 + wl*32 + l31   (the layout of chan_gemm_f32_kernel: same epilogues)
  const int l = l0 + wl * 32 + l31;
  float* Yb = Y ? Y + (size_t)b * y_bstride : nullptr;
  if (epi == 3) {
    __syncthreads();
    float* red = (float*)Xh;                           // 64 n x 2 halves of partial sums
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int nl = wn * 32 + 8 * (r >> 2) + 4 * hi + (r & 3), n = n0 + nl;
      float v = 0.f;
      if (n < N && l < L) v = 1.0f / (1.0f + __expf(-(acc[r] + (bias ? bias[n] : 0.f))));
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (l31 == 0) red[nl * 2 + wl] = v;
    }
    __syncthreads();
    if (tid < 64 && n0 + tid < N) part[((size_t)b * gridDim.x + blockIdx.x) * N + n0 + tid] = red[tid * 2] + red[tid * 2 + 1];
    return;
  }
  if (l >= L) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wn * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
    if (n >= N) continue;
    float v = acc[r] + (bias ? bias[n] : 0.f);
    float* yp = Yb + (size_t)n * ldy + l;
    if (epi == 1) v += *yp;
    else if (epi == 2) v = v > 0.f ? v : 0.f;
    *yp = v;
  }
}


// ---- the gate's two GEMMs, wide form (round 5) -----------------------------------------------------------------------------------------
// chan_gemm_split_kernel above re-stages and re-splits the X tile once per 64-row block of N (2 x for the gate's first GEMM, 8 x for the
// second) and splits its W block in every workgroup: 84 us per launch where the bytes are 40 us' worth. Here a workgroup owns a 64-position
// tile for ALL of N: X is split once per workgroup (XRES: K <= 128, the whole [K, 64] tile resident in LDS; otherwise one 64-deep chunk
// at a time), W comes from bf16 hi / lo images split ONCE per call (duan_stats_kernel's first batch row does it on the side) and is read
// as MFMA fragments straight from global memory -- a lane's 8 consecutive k of its row are 16 contiguous bytes, L2-resident after the
// first workgroups -- one step (128 rows of N x 64 of K) ahead of its MFMAs. Wave w = rows [g * 128 + 32 w, + 32) of group g, both
// 32-position halves. Needs N % 128 == 0, K % 64 == 0.
template <bool XRES, int EPI, int LT>
__global__ __launch_bounds__(256) void chan_gemm_wide_kernel(const float* __restrict__ X, long x_bstride, int ldx, const uint16_t* __restrict__ Wh,
                                                             const uint16_t* __restrict__ Wl, const float* __restrict__ bias, float* __restrict__ Y,
                                                             long y_bstride, int ldy, int N, int K, int L, float* __restrict__ part,
                                                             float* __restrict__ xsum) {
  // A workgroup owns 64 * LT positions (LT = 2 halves the L2 traffic of the W fragments, which every workgroup reads in full).
  // xsum (!XRES only; may be null): [B][ceil(L / 64)][K] sums of X over each 64 positions, per k -- the DUAN's mean of its condition
  // per channel falls out of the gate's first GEMM, which reads every element of it anyway (duan_stats_kernel then reads x alone)
  constexpr int NX = XRES ? 2 : 1;                     // 64-deep chunks of X resident at once
  __shared__ __attribute__((aligned(16))) uint16_t Xh[NX * LT * 64 * CS_LD], Xl[NX * LT * 64 * CS_LD];
  const int b = blockIdx.y, l0 = blockIdx.x * (64 * LT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const float* Xb = X + (size_t)b * x_bstride;
  const int nchunk = K / CS_KC, nstep = nchunk * (N / 128);
  const int xl_s = tid & 63, xk_s = (tid >> 6) * 16;
  auto fetch_x = [&](int k0, float (&xr)[LT][16]) {
#pragma unroll
    for (int t = 0; t < LT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) xr[t][j] = l0 + t * 64 + xl_s < L ? Xb[(size_t)(k0 + xk_s + j) * ldx + l0 + t * 64 + xl_s] : 0.f;
  };
  auto store_x = [&](int slot, const float (&xr)[LT][16]) {
#pragma unroll
    for (int t = 0; t < LT; ++t) {
      u32x4 h[2], l[2];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint16_t a = f32_to_bf16(xr[t][2 * q]), c = f32_to_bf16(xr[t][2 * q + 1]);
        h[q >> 2][q & 3] = (uint32_t)a | ((uint32_t)c << 16);
        l[q >> 2][q & 3] = pack_bf16x2(xr[t][2 * q] - bf16_to_f32(a), xr[t][2 * q + 1] - bf16_to_f32(c));
      }
      uint16_t* dh = Xh + ((slot * LT + t) * 64 + xl_s) * CS_LD + xk_s;
      uint16_t* dl = Xl + ((slot * LT + t) * 64 + xl_s) * CS_LD + xk_s;
      *(u32x4*)dh = h[0]; *(u32x4*)(dh + 8) = h[1];
      *(u32x4*)dl = l[0]; *(u32x4*)(dl + 8) = l[1];
    }
  };
  // W fragments of step s = (group g = s / nchunk, chunk c = s % nchunk): 4 k-steps x {hi, lo}
  auto fetch_w = [&](int s, bf16x8 (&w)[4][2]) {
    const int g = s / nchunk, c = s - g * nchunk;
    const size_t o = (size_t)(g * 128 + wave * 32 + l31) * K + c * CS_KC + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      w[ks][0] = *(const bf16x8*)(Wh + o + ks * 16);
      w[ks][1] = *(const bf16x8*)(Wl + o + ks * 16);
    }
  };
  f32x16 acc[2 * LT];
  const int l_lo = l0 + l31;                           // this lane's position in 32-position block 0; block h = + 32 h
  float* Yb = Y ? Y + (size_t)b * y_bstride : nullptr;
  bf16x8 wa[4][2], wb[4][2];
  float xr[LT][16];
  fetch_w(0, wa);
  if constexpr (XRES) {
    float xr2[LT][16];
    fetch_x(0, xr);
    if (nchunk > 1) fetch_x(CS_KC, xr2);
    store_x(0, xr);
    if (nchunk > 1) store_x(1, xr2);
    __syncthreads();
  } else {
    fetch_x(0, xr);
  }
  auto do_step = [&](const int s, bf16x8 (&wc)[4][2], bf16x8 (&wn)[4][2]) {
    const int g = s / nchunk, c = s - g * nchunk;
    if constexpr (!XRES) {
      __syncthreads();                                 // the previous chunk's fragments have been read
      store_x(0, xr);
      if (xsum && g == 0) {                            // (out-of-range positions were loaded as 0)
#pragma unroll
        for (int t = 0; t < LT; ++t) {                  // one row per 64 positions, as for `part`
          float mine = 0.f;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float tot = wave_total(xr[t][j]);
            mine = lane == j ? tot : mine;
          }
          if (lane < 16 && l0 + 64 * t < L) xsum[((size_t)b * ((L + 63) / 64) + blockIdx.x * LT + t) * K + c * CS_KC + xk_s + lane] = mine;
        }
      }
      __syncthreads();
      if (s + 1 < nstep) fetch_x(((s + 1) % nchunk) * CS_KC, xr);     // the next chunk's loads fly under this chunk's MFMAs
    }
    if (s + 1 < nstep) fetch_w(s + 1, wn);
    if (c == 0) {
#pragma unroll
      for (int h = 0; h < 2 * LT; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][r] = 0.f;
    }
    const int bo = (XRES ? c : 0) * (LT * 64) * CS_LD + l31 * CS_LD + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int h = 0; h < 2 * LT; ++h) {
        const bf16x8 bh = *(const bf16x8*)(Xh + bo + h * 32 * CS_LD + ks * 16), bl = *(const bf16x8*)(Xl + bo + h * 32 * CS_LD + ks * 16);
        acc[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ks][0], bl, acc[h], 0, 0, 0);       // small terms first
        acc[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ks][1], bh, acc[h], 0, 0, 0);
        acc[h] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ks][0], bh, acc[h], 0, 0, 0);
      }
    }
    if (c == nchunk - 1) {
      // acc[h][r]: n = nb + 8*(r/4) + 4*hi + r%4 ; l = l_lo + 32 h
      const int nb = g * 128 + wave * 32;
      f32x4 bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[q] = bias ? *(const f32x4*)(bias + nb + 8 * q + 4 * hi) : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (EPI == 3) {
        // one row of `part` per 64 positions whatever LT is, summed in the same order: the result does not depend on the tile a launch
        // shape chose (a data-parallel shard of another batch size reproduces the full batch bit for bit)
#pragma unroll
        for (int t = 0; t < LT; ++t) {
          float sg[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float bb = bv[r >> 2][r & 3];
            const float s0 = __builtin_amdgcn_rcpf(1.0f + __expf(-(acc[2 * t][r] + bb))), s1 = __builtin_amdgcn_rcpf(1.0f + __expf(-(acc[2 * t + 1][r] + bb)));
            sg[r] = (l_lo + 64 * t < L ? s0 : 0.f) + (l_lo + 64 * t + 32 < L ? s1 : 0.f);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) sg[r] = half_wave_sum_hi16(sg[r]);
          if (l31 == 16 && l0 + 64 * t < L) {
            float* pp = part + ((size_t)b * ((L + 63) / 64) + blockIdx.x * LT + t) * N + nb + 4 * hi;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(pp + 8 * q) = f32x4{sg[4 * q], sg[4 * q + 1], sg[4 * q + 2], sg[4 * q + 3]};
          }
        }
      } else {
#pragma unroll
        for (int h = 0; h < 2 * LT; ++h) {
          const int l = l_lo + 32 * h;
          if (l < L) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float v = acc[h][r] + bv[r >> 2][r & 3];
              float* yp = Yb + (size_t)(nb + 8 * (r >> 2) + 4 * hi + (r & 3)) * ldy + l;
              if constexpr (EPI == 1) v += *yp;
              if constexpr (EPI == 2) v = v > 0.f ? v : 0.f;
              *yp = v;
            }
          }
        }
      }
    }
  };
  for (int s = 0; s < nstep; s += 2) {                 // fragment registers ping-pong: no copy (a copy would wait for the X loads in flight too)
    do_step(s, wa, wb);
    if (s + 1 < nstep) do_step(s + 1, wb, wa);
  }
}

// fp32 [n] -> bf16 hi / lo images (x = hi + lo to 2^-17): what chan_gemm_wide_kernel reads as W
__device__ __forceinline__ void split_bf16_store(const float* __restrict__ src, uint16_t* __restrict__ dh, uint16_t* __restrict__ dl, int i, int n) {
  if (i >= n) return;
  const float v = src[i];
  const uint16_t h = f32_to_bf16(v);
  dh[i] = h;
  dl[i] = f32_to_bf16(v - bf16_to_f32(h));
}
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ a, uint16_t* __restrict__ ah, uint16_t* __restrict__ al, int na,
                                                         const float* __restrict__ b, uint16_t* __restrict__ bh, uint16_t* __restrict__ bl, int nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  split_bf16_store(a, ah, al, i, na);
  split_bf16_store(b, bh, bl, i, nb);
}

}  // namespace

// internal (dgf.hip): the split-bf16 form of lx_chan_gemm_f32, same arguments and epilogues, relative error ~2^-16 instead of exact fp32 products
int lx_chan_gemm_split(const float* X, long x_bstride, int ldx, const float* W, int ldw, const float* bias, float* Y, long y_bstride, int ldy,
                       int B, int N, int K, int L, int epilogue, float* part, void* stream) {
  LX_CHECK_ARG(X && W && B > 0 && N > 0 && K > 0 && L > 0, "lx_chan_gemm_split: bad arguments");
  LX_CHECK_ARG(epilogue >= 0 && epilogue <= 3 && (epilogue == 3 ? part != nullptr : Y != nullptr), "lx_chan_gemm_split: epilogue 0..3 (3 needs part, the others Y)");
  LX_CHECK_ARG(K % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)W & 15) == 0, "lx_chan_gemm_split: K, ldw must be multiples of 4, W 16-byte aligned");
  hipLaunchKernelGGL(chan_gemm_split_kernel, dim3((L + 63) / 64, (N + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, X, x_bstride, ldx, W, ldw, bias, Y,
                     y_bstride, ldy, N, K, L, epilogue, part);
  LX_LAUNCH_CHECK("lx_chan_gemm_split");
  return LX_OK;
}

// internal (dgf.hip): the wide form; Wh / Wl = bf16 hi / lo images of W [N, K] (lx_split_bf16_pair). N % 128 == 0, K % 64 == 0.
// xsum: null, or [B][ceil(L / 64)][K] sums of X over each 64 positions (K > 128 only); part rows likewise per 64 positions, whatever `tile`.
// positions per workgroup for the resident-X form (K <= 128; = the tile the `part` rows are sums over): 128 when that still leaves two
// workgroups per CU -- half the L2 traffic of the W fragments (57 -> 46 us on the gate's second GEMM). The streaming form (K > 128) is
// better off with 64: at 128 its 280 registers leave one wave per SIMD to hide the HBM latency of X (65 -> 70 us).
int lx_chan_gemm_wide_tile(int B, int L) { return (long)B * ((L + 127) / 128) >= 512 ? 128 : 64; }
int lx_chan_gemm_wide(const float* X, long x_bstride, int ldx, const uint16_t* Wh, const uint16_t* Wl, const float* bias, float* Y, long y_bstride,
                      int ldy, int B, int N, int K, int L, int epilogue, float* part, float* xsum, int tile, void* stream) {
  LX_CHECK_ARG(tile == 64 || tile == 128, "lx_chan_gemm_wide: tile = 64 or 128 positions per workgroup");
  LX_CHECK_ARG(!xsum || K > 128, "lx_chan_gemm_wide: xsum needs the streaming form (K > 128)");
  LX_CHECK_ARG(X && Wh && Wl && B > 0 && L > 0 && N > 0 && N % 128 == 0 && K > 0 && K % 64 == 0, "lx_chan_gemm_wide: N %% 128, K %% 64 (N=%d K=%d)", N, K);
  LX_CHECK_ARG(epilogue >= 0 && epilogue <= 3 && (epilogue == 3 ? part != nullptr : Y != nullptr), "lx_chan_gemm_wide: epilogue 0..3 (3 needs part, the others Y)");
  LX_CHECK_ARG(N % 4 == 0 && (!bias || ((uintptr_t)bias & 15) == 0) && (epilogue != 3 || ((uintptr_t)part & 15) == 0), "lx_chan_gemm_wide: bias / part must be 16-byte aligned");
  const int lt = tile / 64;
  const dim3 grid((L + 64 * lt - 1) / (64 * lt), B);
  hipStream_t st = (hipStream_t)stream;
#define LX_WIDE3(XR, EP, LT_) hipLaunchKernelGGL((chan_gemm_wide_kernel<XR, EP, LT_>), grid, dim3(256), 0, st, X, x_bstride, ldx, Wh, Wl, bias, Y, y_bstride, ldy, N, K, L, part, xsum)
#define LX_WIDE(XR, EP) do { if (lt == 2) LX_WIDE3(XR, EP, 2); else LX_WIDE3(XR, EP, 1); } while (0)
  const bool xres = K <= 128;
  switch (epilogue) {
    case 0: if (xres) LX_WIDE(true, 0); else LX_WIDE(false, 0); break;
    case 1: if (xres) LX_WIDE(true, 1); else LX_WIDE(false, 1); break;
    case 2: if (xres) LX_WIDE(true, 2); else LX_WIDE(false, 2); break;
    default: if (xres) LX_WIDE(true, 3); else LX_WIDE(false, 3); break;
  }
#undef LX_WIDE3
#undef LX_WIDE
  LX_LAUNCH_CHECK("lx_chan_gemm_wide");
  return LX_OK;
}
int lx_split_bf16_pair(const float* a, uint16_t* ah, uint16_t* al, int na, const float* b, uint16_t* bh, uint16_t* bl, int nb, void* stream) {
  hipLaunchKernelGGL(split_bf16_kernel, dim3((max(na, nb) + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, ah, al, na, b, bh, bl, nb);
  LX_LAUNCH_CHECK("lx_split_bf16_pair");
  return LX_OK;
}

extern "C" int lx_chan_gemm_f32(const float* X, long x_bstride, int ldx, const float* W, int ldw, const float* bias, float* Y, long y_bstride,
                                int ldy, int B, int N, int K, int L, int epilogue, float* part, void* stream) {
  LX_CHECK_ARG(X && W && B > 0 && N > 0 && K > 0 && L > 0, "lx_chan_gemm_f32: bad arguments");
  LX_CHECK_ARG(epilogue >= 0 && epilogue <= 3 && (epilogue == 3 ? part != nullptr : Y != nullptr), "lx_chan_gemm_f32: epilogue 0..3 (3 needs part, the others Y)");
  LX_CHECK_ARG(K % 4 == 0 && ldw % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0, "lx_chan_gemm_f32: K, ldw, ldx must be multiples of 4, X / W 16-byte aligned");
  hipLaunchKernelGGL(chan_gemm_f32_kernel, dim3((L + 63) / 64, (N + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, X, x_bstride, ldx, W, ldw, bias, Y,
                     y_bstride, ldy, N, K, L, epilogue, part);
  LX_LAUNCH_CHECK("lx_chan_gemm_f32");
  return LX_OK;
}

static bool env_mw() {          // LX_S4_MULTIWAVE=0 forces the one-wave-per-sequence kernel (A/B, tests); read per call: the op runs ~10x per image
  const char* e = getenv("LX_S4_MULTIWAVE");
  return !e || atoi(e) != 0;
}

extern "C" int lx_s4_scan(const float* u, const double* lam, const double* w, const float* Dskip, float* y, int B, int H, int L,
                          int N, void* stream) {
  LX_CHECK_ARG(u && lam && w && Dskip && y, "lx_s4_scan: NULL operand");
  LX_CHECK_ARG(B > 0 && H > 0 && N > 0 && L >= 64 && L % 64 == 0, "lx_s4_scan: L=%d must be a positive multiple of 64", L);
  const int ch = L / 64;
  const dim3 grid(B * H), block(64);
  hipStream_t s = (hipStream_t)stream;
  // four (two) waves per sequence wherever L allows it -- for every batch size, so that a sample's result does not depend on
  // how many other samples share the launch (data-parallel shards == the single-GPU batch, bit for bit)
  if (env_mw()) {
    bool done = true;
    if (L % 256 == 0 && L / 256 == 16) hipLaunchKernelGGL((s4_scan_mw_kernel<16, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L % 256 == 0 && L / 256 == 8) hipLaunchKernelGGL((s4_scan_mw_kernel<8, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L % 256 == 0 && L / 256 == 4) hipLaunchKernelGGL((s4_scan_mw_kernel<4, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L % 256 == 0 && L / 256 == 2) hipLaunchKernelGGL((s4_scan_mw_kernel<2, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L == 8192) hipLaunchKernelGGL((s4_scan_mw_kernel<32, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L == 256) hipLaunchKernelGGL((s4_scan_mw_kernel<1, 4>), grid, dim3(256), 0, s, u, lam, w, Dskip, y, H, L, N);
    else if (L == 128) hipLaunchKernelGGL((s4_scan_mw_kernel<1, 2>), grid, dim3(128), 0, s, u, lam, w, Dskip, y, H, L, N);
    else done = false;
    if (done) {
      LX_LAUNCH_CHECK("lx_s4_scan");
      return LX_OK;
    }
  }
#define LX_SCAN_CASE(C) case C: hipLaunchKernelGGL(s4_scan_kernel<C>, grid, block, 0, s, u, lam, w, Dskip, y, H, L, N); break;
  switch (ch) {
    LX_SCAN_CASE(1) LX_SCAN_CASE(2) LX_SCAN_CASE(4) LX_SCAN_CASE(8) LX_SCAN_CASE(16) LX_SCAN_CASE(32) LX_SCAN_CASE(64)
    default: lx_set_error("lx_s4_scan: L/64=%d must be a power of two <= 64", ch); return LX_ERR_UNSUPPORTED;
  }
#undef LX_SCAN_CASE
  LX_LAUNCH_CHECK("lx_s4_scan");
  return LX_OK;
}

extern "C" int lx_s4_conv(const float* u, const float* Kker, const float* Dskip, float* y, int B, int H, int L, void* stream) {
  LX_CHECK_ARG(u && Kker && Dskip && y && B > 0 && H > 0 && L > 0, "lx_s4_conv: bad arguments");
  LX_CHECK_ARG(L <= 8192, "lx_s4_conv: L=%d exceeds the 8192 LDS-resident limit", L);
  hipLaunchKernelGGL(s4_conv_kernel, dim3(B * H), dim3(256), 2 * L * sizeof(float), (hipStream_t)stream, u, Kker, Dskip, y, H, L);
  LX_LAUNCH_CHECK("lx_s4_conv");
  return LX_OK;
}

extern "C" int lx_chanmix(const float* x, const float* W, const float* bias, const float* resid, const float* ln_g,
                          const float* ln_b, float* y, int B, int Hin, int Hout, int L, int act, void* stream) {
  LX_CHECK_ARG(x && W && y && B > 0 && L > 0, "lx_chanmix: bad arguments");
  LX_CHECK_ARG((ln_g == nullptr) == (ln_b == nullptr), "lx_chanmix: LayerNorm gamma/beta must come together");
  const dim3 grid((L + 255) / 256, B), block(256);
  hipStream_t s = (hipStream_t)stream;
#define LX_CM(I, O) if (Hin == I && Hout == O) { hipLaunchKernelGGL((chanmix_kernel<I, O>), grid, block, 0, s, x, W, bias, resid, ln_g, ln_b, y, L, act); } else
  LX_CM(4, 64) LX_CM(64, 64) LX_CM(4, 4) LX_CM(6, 6) {
    lx_set_error("lx_chanmix: (Hin,Hout)=(%d,%d) unsupported; CS3 uses (4,64),(64,64),(4,4),(6,6)", Hin, Hout);
    return LX_ERR_UNSUPPORTED;
  }
#undef LX_CM
  LX_LAUNCH_CHECK("lx_chanmix");
  return LX_OK;
}

extern "C" int lx_pyramid_pool(const float* x, float* y, int B, int C, int L, const int* sizes, int n_sizes, int ldy, int y_col0,
                               void* stream) {
  LX_CHECK_ARG(x && y && sizes && n_sizes >= 1 && n_sizes <= 8, "lx_pyramid_pool: 1..8 output sizes required");
  PoolSizes ps;
  ps.n = n_sizes;
  int off = 0;
  for (int i = 0; i < n_sizes; ++i) {
    LX_CHECK_ARG(sizes[i] >= 1, "lx_pyramid_pool: size[%d]=%d", i, sizes[i]);
    ps.size[i] = sizes[i];
    ps.off[i] = off;
    off += sizes[i];
  }
  ps.off[n_sizes] = off;
  LX_CHECK_ARG(ldy >= y_col0 + off, "lx_pyramid_pool: ldy=%d too small for %d columns at %d", ldy, off, y_col0);
  const size_t total = (size_t)B * C * off;
  hipLaunchKernelGGL(pyramid_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, B * C, L, ps, ldy, y_col0);
  LX_LAUNCH_CHECK("lx_pyramid_pool");
  return LX_OK;
}

extern "C" int lx_layernorm_relu(float* x, const float* g, const float* b, int M, int D, float eps, void* stream) {
  LX_CHECK_ARG(x && g && b && M > 0 && D > 0, "lx_layernorm_relu: bad arguments");
  hipLaunchKernelGGL(layernorm_relu_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, x, g, b, D, eps);
  LX_LAUNCH_CHECK("lx_layernorm_relu");
  return LX_OK;
}

extern "C" int lx_linear_f32(const float* X, int ldx, int x_trans, const float* W, int ldw, const float* bias, float* Y, int ldy,
                             int y_trans, int M, int N, int K, int accumulate, void* stream) {
  LX_CHECK_ARG(X && W && Y && M > 0 && N > 0 && K > 0, "lx_linear_f32: bad arguments");
  if (M <= 16 && !x_trans && !y_trans && K >= 256 && K % 4 == 0 && ldx % 4 == 0 && ldw % 4 == 0 && (((uintptr_t)X | (uintptr_t)W) & 15) == 0) {
    // a few rows against a big weight: stream the weights once at HBM rate instead of tiling a 64-row problem that is 3/4 padding
    const dim3 g((N + 7) / 8), blk(256);
    if (M <= 4) hipLaunchKernelGGL(linear_f32_skinny_kernel<4>, g, blk, 0, (hipStream_t)stream, X, ldx, W, ldw, bias, Y, ldy, M, N, K, accumulate);
    else hipLaunchKernelGGL(linear_f32_skinny_kernel<16>, g, blk, 0, (hipStream_t)stream, X, ldx, W, ldw, bias, Y, ldy, M, N, K, accumulate);
    LX_LAUNCH_CHECK("lx_linear_f32");
    return LX_OK;
  }
  const dim3 grid((N + 63) / 64, (M + 63) / 64), block(256);
  hipLaunchKernelGGL(linear_f32_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, x_trans, W, ldw, bias, Y, ldy, y_trans, M, N, K, accumulate);
  LX_LAUNCH_CHECK("lx_linear_f32");
  return LX_OK;
}
