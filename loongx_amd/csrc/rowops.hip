// rowops.hip -- HBM-bound row kernels of the DiT step (gfx950): AdaLN LayerNorm+modulate, per-head
// RMSNorm+RoPE(+V^T image), LoRA down-projection, skinny (M<=16) linears, timestep embedding. (The scheduler step: step.hip.)
// All loads/stores are 8-16 B per lane and coalesced; reductions are wave64 shuffles (no LDS, no atomics).
#include "row_common.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------------
// LayerNorm(no affine) + (1+scale)*x + shift, fp32 in -> bf16 out. One wave per row, row kept in VGPRs.
// Reference: AdaLayerNormZero/ZeroSingle/Continuous + norm2 modulation (block.py:192-207,238-253,301,305).
// ------------------------------------------------------------------------------------------------------
// LM (round 5): the rows [lora_row0, lora_row0 + lora_rows) (the streams that run with the adapter on) also get their LoRA down-projection
// T[row - lora_row0, 0..R) = Y_row . Adown[R, D]^T (R <= 16) on the matrix pipe while the workgroup's four normalised rows are at hand:
// the rows go to LDS as the 16-bit operand images they are stored as, Adown is the MFMA "A" operand (rows = r), the four rows the "B"
// operand (columns m = 0..3 of 16, the others zero), the four waves split K and add their partial tiles through LDS -- the same operands
// and instruction as lora_down_mfma_kernel, another split of K (results agree to fp32 summation order). The separate lx_lora_down
// launch over the same rows (6.7 us, 76 of the 132 per denoise step sit behind a LayerNorm) disappears; workgroups without adapter rows
// take the plain path (the decision is workgroup-uniform). Rounds 2-4 had a vector-ALU form of this (576-768 FMAs and 12-16 ds_bpermute
// wave reductions per row): 1.1 % slower per image than the separate launches, never enabled.
struct LnLora { const uint16_t* A; float* T; int R, ldt, row0, rows; };

// F16: Y is the fp16 operand image of an LX_OPERANDS_F16 GEMM (nearest even, saturated to +-65504; *f16_ovf counts the waves that clipped).
template <int NCH, bool LM = false, bool F16 = false>  // D = NCH*256: lane owns float4 chunks lane, lane+64, ...
__global__ __launch_bounds__(256, 3) void ln_modulate_kernel(const float* __restrict__ X, int ldx, const LnSegs segs, int mod_ld,
                                                          uint16_t* __restrict__ Y, int ldy, int M, int D, float eps, const LnLora lo = LnLora{},
                                                          int* __restrict__ f16_ovf = nullptr) {
  constexpr int RS = NCH * 256 + 32;                    // LDS row stride (elements): + 64 B, so the four rows' fragments fall on distinct banks
  __shared__ __attribute__((aligned(16))) uint16_t rows_s[LM ? 4 * RS : 8];
  __shared__ f32x4 red_s[LM ? 4 * 64 : 1];
  const int wave = threadIdx.x >> 6;
  const int row_l = blockIdx.x * 4 + wave;              // row in launch order
  if constexpr (!LM) {
    if (row_l >= M) return;
  }
  const bool valid = row_l < M;
  auto phys = [&](int rl, int& sg_o, int& rin_o) {      // launch-order row -> (segment, row in segment) -> physical row
    int sg = 0, acc_rows = 0;
    while (sg < segs.n - 1 && rl >= acc_rows + segs.n_rows[sg]) { acc_rows += segs.n_rows[sg]; ++sg; }
    sg_o = sg; rin_o = rl - acc_rows;
    return segs.row0[sg] + rin_o;
  };
  int sg, rin;
  const int row = phys(min(row_l, M - 1), sg, rin);
  bool wg_lora = false;                                 // workgroup-uniform: one of its four rows runs the adapter
  if constexpr (LM) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int rl = blockIdx.x * 4 + w;
      int s2, r2;
      const int pr = phys(min(rl, M - 1), s2, r2);
      wg_lora |= rl < M && pr >= lo.row0 && pr < lo.row0 + lo.rows;
    }
  }
  const float* shift = segs.shift[sg];
  const float* scale = segs.scale[sg];
  const int rows_per_batch = segs.rows_per_batch[sg];
  const int lane = threadIdx.x & 63;
  const float* xr = X + (size_t)row * ldx;
  f32x4 v[NCH];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) v[i] = *(const f32x4*)(xr + (i * 64 + lane) * 4);
  // the modulation rows do not depend on the statistics: their loads go out with the row's (one memory round trip instead of two: the
  // kernel has 2.5 workgroups per CU at S = 2560 and is bound by its own latency chain, 11 us per launch in the step, 76 launches)
  const int b = rin / rows_per_batch;
  const float* sh = shift + (size_t)b * mod_ld;
  const float* sc = scale + (size_t)b * mod_ld;
  f32x4 av[NCH], bv[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    av[i] = *(const f32x4*)(sc + (i * 64 + lane) * 4);
    bv[i] = *(const f32x4*)(sh + (i * 64 + lane) * 4);
  }
  // (hipcc sinks most of these loads below the first reduction again -- 144 registers of loads in flight do not fit the 168 that three
  //  waves per SIMD allow without spilling; pinning them with an empty asm was tried: 2-19 spilled registers per variant. What reaches
  //  the memory system early is what fits.)
#pragma unroll
  for (int i = 0; i < NCH; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_total(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = v[i][c] - mean;
      q += d * d;
    }
  const float rstd = rsqrtf(wave_total(q) / (float)D + eps);
  uint16_t* yr = Y + (size_t)row * ldy;
  float f16_mx = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int col = (i * 64 + lane) * 4;
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (v[i][c] - mean) * rstd * (1.0f + av[i][c]) + bv[i][c];
    u32x2 w;
    w[0] = pack_op16x2<F16>(o[0], o[1], f16_mx);
    w[1] = pack_op16x2<F16>(o[2], o[3], f16_mx);
    if (valid) *(u32x2*)(yr + col) = w;
    if constexpr (LM) {
      if (wg_lora) *(u32x2*)(rows_s + wave * RS + col) = w;
    }
  }
  if constexpr (LM) {
    if (wg_lora) {
      // K = NCH * 256 in 32-deep MFMA steps; wave w takes steps w, w + 4, ... (2 NCH of them). Adown fragments straight from global
      // memory (L2-resident: every workgroup of the launch reads the same R rows), all in flight before the barrier.
      constexpr int NS = 2 * NCH, NB = NS >= 8 ? NS / 2 : NS;     // two batches of fragments: 176 registers (one batch) would leave two waves
      const int l15 = lane & 15, kq = lane >> 4;                  // per SIMD, and the launch is 2.5 workgroups per CU: a second round
      const uint16_t* ap = lo.A + (size_t)min(l15, lo.R - 1) * D + kq * 8;
      __builtin_amdgcn_sched_barrier(0);          // (hipcc would hoist these loads above the row's arithmetic: 176 registers again)
      bf16x8 af[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) af[u] = *(const bf16x8*)(ap + (4 * u + wave) * 32);
      __syncthreads();
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const uint16_t* xp = rows_s + (l15 & 3) * RS + kq * 8;
      const bf16x8 zero = {};
#pragma unroll
      for (int u0 = 0; u0 < NS; u0 += NB) {
        if (u0 > 0) {
#pragma unroll
          for (int u = 0; u < NB; ++u) af[u] = *(const bf16x8*)(ap + (4 * (u0 + u) + wave) * 32);
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          bf16x8 xf = *(const bf16x8*)(xp + (4 * (u0 + u) + wave) * 32);
          xf = l15 < 4 ? xf : zero;
          if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, af[u]), __builtin_bit_cast(f16x8, xf), acc, 0, 0, 0);
          else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u], xf, acc, 0, 0, 0);
        }
      }
      red_s[wave * 64 + lane] = acc;                  // acc[j]: r = 4 kq + j, row m = l15 (< 4 are real)
      __syncthreads();
      if (threadIdx.x < 64) {
        const int m = threadIdx.x >> 4, r = threadIdx.x & 15;
        const float* rp = (const float*)red_s + (m + 16 * (r >> 2)) * 4 + (r & 3);
        const float t = ((rp[0] + rp[256]) + rp[512]) + rp[768];
        const int rl = blockIdx.x * 4 + m;
        int s2, r2;
        const int pr = phys(min(rl, M - 1), s2, r2);
        if (rl < M && r < lo.R && pr >= lo.row0 && pr < lo.row0 + lo.rows) lo.T[(size_t)(pr - lo.row0) * lo.ldt + r] = t;
      }
    }
  }
  if constexpr (F16) report_f16_overflow(f16_mx, f16_ovf);
}

// generic D (multiple of 4): the three-pass row body of row_common.h, 16-bit operand store
template <bool F16 = false>
__global__ __launch_bounds__(256) void ln_modulate_generic(const float* __restrict__ X, int ldx, const LnSegs segs, int mod_ld,
                                                           uint16_t* __restrict__ Y, int ldy, int M, int D, float eps, int* __restrict__ f16_ovf = nullptr) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6), rin, sg;
  if (!ln_row(segs, M, row, rin, sg)) return;
  const int lane = threadIdx.x & 63;
  const float* xr = X + (size_t)row * ldx;
  float mean, rstd;
  ln_row_stats(xr, D, lane, mean, rstd, eps);
  const float *sc, *sh;
  ln_mod_rows(segs, sg, rin, mod_ld, sc, sh);
  uint16_t* yr = Y + (size_t)row * ldy;
  float f16_mx = 0.f;
  ln_emit(xr, sc, sh, D, lane, mean, rstd, [&](int c, const float (&o)[4]) {
    u32x2 w;
    w[0] = pack_op16x2<F16>(o[0], o[1], f16_mx);
    w[1] = pack_op16x2<F16>(o[2], o[3], f16_mx);
    *(u32x2*)(yr + c) = w;
  });
  if constexpr (F16) report_f16_overflow(f16_mx, f16_ovf);
}

// ------------------------------------------------------------------------------------------------------
// Q/K: RMSNorm(128, weight) + RoPE in place; V -> V^T image. Block = 64 positions x 1 head x 1 batch.
// 16 lanes own one (row, head) vector of 128 bf16 (8 elements = 4 rotary pairs each). Tile decode, arithmetic
// and the general pass loop: row_common.h.
// ------------------------------------------------------------------------------------------------------

// FAST: every segment has norm_q / norm_k weights and RoPE tables (the DiT case). The launch is one resident generation of waves
// (3840 waves on 1024 SIMDs at S = 2560), so its duration is the length of one thread's dependent chain of memory round trips,
// not bandwidth. The FAST body therefore issues all loads of two of the thread's four rows (q, k, v chunks, RoPE table rows) before
// anything is computed or stored -- the q / k stores go to the buffer the next rows' loads read, so hipcc cannot hoist them
// itself -- without branches in between (at a control-flow join its wait-count pass falls back to vmcnt(0)).
// IN_F16: the projection launch stored IEEE fp16 (an LX_OPERANDS_F16 16-bit store without LX_EPI_QKV: stream lengths the fused epilogue does
// not take, or callers that asked for the separate pass). q / k are read as fp16 and written back in place as bf16 -- what the attention
// kernels read --, V goes to the V^T image rounded fp16 -> bf16. Only the general (non-FAST) body has this form: the path is the rare one.
__device__ __forceinline__ void unpack16x8(const u32x4 raw, float* x, bool in_f16) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (in_f16) {
      x[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw[i] & 0xffffu));
      x[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(raw[i] >> 16));
    } else {
      x[2 * i] = __uint_as_float(raw[i] << 16);
      x[2 * i + 1] = __uint_as_float(raw[i] & 0xffff0000u);
    }
  }
}
__device__ __forceinline__ u32x4 f16x8_to_bf16x8(const u32x4 raw) {
  float x[8];
  unpack16x8(raw, x, true);
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(x[2 * i], x[2 * i + 1]);
  return o;
}

// The 16-bit source of the general pass loop (qkv_prep_rows): bf16 or fp16 q / k / v chunks of QKV [rows, ld], zeros for rows past the
// end; V goes to the transpose buffer as bf16. The lane's chunk of a row is at h * 128 + sub * 8.
template <bool IN_F16>
struct Qkv16Src {
  const uint16_t* QKV; int ld, q_col, k_col, v_col, h, sub, rloc;
  uint16_t (*vt_s)[128 + 8];
  const uint16_t* rowp;
  __device__ __forceinline__ void row(size_t r) { rowp = QKV + r * ld + h * 128 + sub * 8; }
  __device__ __forceinline__ u32x4 chunk(int col, bool valid) const {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (valid) raw = *(const u32x4*)(rowp + col);
    return raw;
  }
  __device__ __forceinline__ void load8(int which, bool valid, float (&x)[8]) const { unpack16x8(chunk(which ? k_col : q_col, valid), x, IN_F16); }
  __device__ __forceinline__ void stash_v(int pass, bool valid) const {
    const u32x4 raw = chunk(v_col, valid);
    *(u32x4*)&vt_s[pass * 16 + rloc][sub * 8] = IN_F16 ? f16x8_to_bf16x8(raw) : raw;
  }
};

// bf16 results: q in place, k in place or (KIMG) to the key image K2; the V stash only when a V^T image is asked for
template <bool IN_F16, bool KIMG>
struct QkvBf16IO : Qkv16Src<IN_F16> {
  uint16_t* K2; int ldk2, k2_col;
  bool vt;
  uint16_t* kdst;
  __device__ __forceinline__ void row(size_t r) {
    Qkv16Src<IN_F16>::row(r);
    if constexpr (KIMG) kdst = K2 + r * ldk2 + k2_col + this->h * 128 + this->sub * 8;
  }
  __device__ __forceinline__ void store8(int which, bool valid, const float (&y)[8]) const {
    if (!valid) return;
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(y[2 * i], y[2 * i + 1]);
    uint16_t* dst = const_cast<uint16_t*>(this->rowp) + (which ? this->k_col : this->q_col);
    if constexpr (KIMG) {
      if (which) dst = kdst;
    }
    *(u32x4*)dst = o;
  }
  __device__ __forceinline__ void stash_v(int pass, bool valid) const {
    if (vt) Qkv16Src<IN_F16>::stash_v(pass, valid);
  }
};

// KIMG (lx_qkv_prep_kv_segs): k goes to the same rows of a key image of its own (K2, head h at k2_col + h*128) and the k columns of QKV stay
// as they are; q is still written in place. Together with the V^T stores below -- only the 64-slot tiles of the launched segments, the tail
// of a segment's last tile zero-filled -- a launch over some segments leaves the other segments' keys and V^T columns alone: the per-layer
// images of a step-invariant condition stream on shapes (or with operands) the fused projection epilogue does not take.
template <bool FAST, bool IN_F16 = false, bool KIMG = false>
__global__ __launch_bounds__(256) void qkv_prep_kernel(uint16_t* __restrict__ QKV, int ld, int q_col, int k_col, int v_col,
                                                       const QkvSegs segs, float eps, uint16_t* __restrict__ VT, int vt_ld, int H,
                                                       uint16_t* __restrict__ K2, int ldk2, int k2_col) {
  __shared__ uint16_t vt_s[64][128 + 8];
  QkvTile t;
  qkv_tile(segs, blockIdx, threadIdx, t);
  const int p0 = t.p0, h = t.h, b = t.b, tid = threadIdx.x, vt_pos0 = segs.vt_pos0[t.sg];
  if constexpr (FAST) {
    // This body keeps its own copy of rms_rope8's arithmetic (row_common.h): written through the helper the values are the same but hipcc
    // hoists the shuffle indices in another order and allocates other registers, and the launch sits on the default denoise step.
    const int rows_per_batch = t.rows_per_batch, sub = t.sub, rloc = t.rloc;
    const float* __restrict__ wq = segs.wq[t.sg];
    const float* __restrict__ wk = segs.wk[t.sg];
    const float* __restrict__ cos_tab = segs.cos_tab[t.sg];
    const float* __restrict__ sin_tab = segs.sin_tab[t.sg];
    const size_t rbase = t.rbase();
    const f32x4 wq0 = *(const f32x4*)(wq + sub * 8), wq1 = *(const f32x4*)(wq + sub * 8 + 4);
    const f32x4 wk0 = *(const f32x4*)(wk + sub * 8), wk1 = *(const f32x4*)(wk + sub * 8 + 4);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      uint16_t* rowp[2];
      uint16_t* kdst[2];
      bool valid[2];
      u32x4 raw[2][3];
      f32x4 cs[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int p = p0 + (half * 2 + u) * 16 + rloc;
        valid[u] = p < rows_per_batch;
        const int pc = valid[u] ? p : 0;          // row 0 of the batch stands in for rows past the end (loaded, never stored)
        rowp[u] = QKV + (rbase + pc) * ld + h * 128 + sub * 8;
        kdst[u] = KIMG ? K2 + (rbase + pc) * ldk2 + k2_col + h * 128 + sub * 8 : rowp[u] + k_col;
        raw[u][0] = *(const u32x4*)(rowp[u] + q_col);
        raw[u][1] = *(const u32x4*)(rowp[u] + k_col);
        raw[u][2] = *(const u32x4*)(rowp[u] + v_col);
        const float* ct = cos_tab + (size_t)pc * 128 + sub * 8;
        const float* st = sin_tab + (size_t)pc * 128 + sub * 8;
        cs[u][0] = *(const f32x4*)ct; cs[u][1] = *(const f32x4*)(ct + 4);
        cs[u][2] = *(const f32x4*)st; cs[u][3] = *(const f32x4*)(st + 4);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        u32x4 out[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) {   // 0: q, 1: k
          float x[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(raw[u][which][i] << 16);
            x[2 * i + 1] = __uint_as_float(raw[u][which][i] & 0xffff0000u);
          }
          float ss = 0.f;
#pragma unroll
          for (int i = 0; i < 8; ++i) ss += x[i] * x[i];
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
          const float r = rsqrtf(ss * (1.0f / 128.0f) + eps);
          const f32x4 w0 = which ? wk0 : wq0, w1 = which ? wk1 : wq1;
#pragma unroll
          for (int i = 0; i < 4; ++i) { x[i] = x[i] * r * w0[i]; x[4 + i] = x[4 + i] * r * w1[i]; }
          float y[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {   // pairs (2i, 2i+1): out = x*cos + rot*sin, rot = (-x_odd, x_even)
            const float ce = i < 2 ? cs[u][0][2 * i] : cs[u][1][2 * i - 4], co = i < 2 ? cs[u][0][2 * i + 1] : cs[u][1][2 * i - 3];
            const float se = i < 2 ? cs[u][2][2 * i] : cs[u][3][2 * i - 4], so = i < 2 ? cs[u][2][2 * i + 1] : cs[u][3][2 * i - 3];
            y[2 * i] = x[2 * i] * ce - x[2 * i + 1] * se;
            y[2 * i + 1] = x[2 * i + 1] * co + x[2 * i] * so;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) out[which][i] = pack_bf16x2(y[2 * i], y[2 * i + 1]);
        }
        if (valid[u]) {
          *(u32x4*)(rowp[u] + q_col) = out[0];
          *(u32x4*)kdst[u] = out[1];
        }
        if (VT) *(u32x4*)&vt_s[(half * 2 + u) * 16 + rloc][sub * 8] = valid[u] ? raw[u][2] : u32x4{0u, 0u, 0u, 0u};
      }
    }
  } else {
    QkvBf16IO<IN_F16, KIMG> io{{QKV, ld, q_col, k_col, v_col, h, t.sub, t.rloc, vt_s, nullptr}, K2, ldk2, k2_col, VT != nullptr, nullptr};
    qkv_prep_rows(segs, t, eps, io);
  }
  if (!VT) return;
  __syncthreads();
  // write V^T rows: thread -> (d, 8 consecutive slots); slot -> source key via the (involutive) interleave
  uint16_t* vtb = VT + ((size_t)(b * H + h) * 128) * vt_ld + vt_pos0 + p0;
  for (int item = tid; item < 128 * 8; item += 256) {
    const int d = item >> 3, g = item & 7;
    uint16_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = vt_s[lx_vt_interleave(g * 8 + i)][d];
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_u16x2(e[2 * i], e[2 * i + 1]);
    *(u32x4*)(vtb + (size_t)d * vt_ld + g * 8) = o;
  }
}

// ------------------------------------------------------------------------------------------------------
// fp8 (OCP e4m3) variant for the fp8 attention path (BASELINE configs[4]): the same RMSNorm + RoPE arithmetic in fp32,
// but q and k go to separate byte images Q8 / K8 [rows, H*128] scaled by q_scale / k_scale, and V to a byte V^T image whose
// 64 keys per tile are in lx_vt8_key order (common.h). The bf16 QKV buffer is left untouched.
// ------------------------------------------------------------------------------------------------------
template <bool IN_F16>
struct QkvFp8IO : Qkv16Src<IN_F16> {
  uint8_t* Q8; uint8_t* K8; int ld8;
  float q_scale, k_scale;
  size_t off8;
  __device__ __forceinline__ void row(size_t r) {
    Qkv16Src<IN_F16>::row(r);
    off8 = r * ld8 + this->h * 128 + this->sub * 8;
  }
  __device__ __forceinline__ void store8(int which, bool valid, const float (&y)[8]) const {
    if (!valid) return;
    const float sc = which ? k_scale : q_scale;
    u32x2 o;
    o[0] = pack_fp8x4(y[0] * sc, y[1] * sc, y[2] * sc, y[3] * sc);
    o[1] = pack_fp8x4(y[4] * sc, y[5] * sc, y[6] * sc, y[7] * sc);
    *(u32x2*)((which ? K8 : Q8) + off8) = o;
  }
};

template <bool IN_F16>
__global__ __launch_bounds__(256) void qkv_prep_fp8_kernel(const uint16_t* __restrict__ QKV, int ld, int q_col, int k_col, int v_col,
                                                           const QkvSegs segs, float eps, uint8_t* __restrict__ Q8,
                                                           uint8_t* __restrict__ K8, int ld8, uint8_t* __restrict__ VT8, int vt_ld,
                                                           int H, float q_scale, float k_scale, float v_scale) {
  __shared__ uint16_t vt_s[64][128 + 8];
  QkvTile t;
  qkv_tile(segs, blockIdx, threadIdx, t);
  QkvFp8IO<IN_F16> io{{QKV, ld, q_col, k_col, v_col, t.h, t.sub, t.rloc, vt_s, nullptr}, Q8, K8, ld8, q_scale, k_scale, 0};
  qkv_prep_rows(segs, t, eps, io);
  __syncthreads();
  // V^T byte image: thread -> (d, 16 consecutive byte positions of the 64-key tile row)
  uint8_t* vtb = VT8 + ((size_t)(t.b * H + t.h) * 128) * vt_ld + segs.vt_pos0[t.sg] + t.p0;
  for (int item = threadIdx.x; item < 128 * 4; item += 256) {
    const int d = item >> 2, c = item & 3;
    float e[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) e[i] = __uint_as_float((uint32_t)vt_s[lx_vt8_key(c * 16 + i)][d] << 16) * v_scale;
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = pack_fp8x4(e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]);
    *(u32x4*)(vtb + (size_t)d * vt_ld + c * 16) = o;
  }
}

// ------------------------------------------------------------------------------------------------------
// LoRA down-projection: T[M,R] = X[M,K] . A[R,K]^T (bf16 in, fp32 out) on v_mfma_f32_16x16x32_bf16. R <= 16: this kernel;
// 16 < R <= 256: lora_down_wide_kernel below.
// Workgroup = 8 waves = 16 rows; the waves split K eight ways and reduce through LDS. A is the MFMA "A"
// operand (rows = r), X the "B" operand (cols = m): each lane ends with 4 consecutive r of one row m.
// ------------------------------------------------------------------------------------------------------
// blockIdx.y = slab: in the K-split form (lx_lora_down) slab s covers K range s; in the multi-term form (lx_lora_down_terms,
// precise mode) slab s is a different (X, A) pair over the whole K -- the cross terms x_hi.A, x_lo.A, x_hi.A_lo in ONE launch.
struct LoraTerms {
  const uint16_t* X[4];
  const uint16_t* A[4];
  int ldx[4];
  int n;                  // 0: K-split form (X[0], A[0]); > 0: one slab per term
};

template <bool F16 = false>      // F16: X and A are fp16 images (the operands of an LX_OPERANDS_F16 GEMM), v_mfma_f32_16x16x32_f16
__global__ __launch_bounds__(512) void lora_down_mfma_kernel(const LoraTerms terms, float* __restrict__ T, int ldt, int M, int K, int R, int Ks,
                                                             int split_stride) {
  __shared__ f32x4 red[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16;
  const int term = terms.n > 0 ? (int)blockIdx.y : 0;
  const uint16_t* __restrict__ X = terms.X[term];
  const uint16_t* __restrict__ A = terms.A[term];
  const int ldx = terms.ldx[term];
  const int kbeg = terms.n > 0 ? 0 : blockIdx.y * Ks, kend = terms.n > 0 ? K : min(K, kbeg + Ks);
  T += (size_t)blockIdx.y * split_stride;
  const int l15 = lane & 15, kq = lane >> 4;
  const uint16_t* xp = X + (size_t)min(m0 + l15, M - 1) * ldx + kq * 8;
  const uint16_t* ap = A + (size_t)min(l15, R - 1) * K + kq * 8;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // A wave's K steps are 256 apart. Written as {load, load, wait, MFMA} per step the loop pays the memory latency once per step (7.5 us
  // per launch in round 2: the whole kernel was that chain); round 3 put up to eight steps' loads in flight, in chunks of 8 / 4 / 2 / 1
  // -- still two to four round trips per wave (3 steps at K = 3072 with four K-split slabs, 12 at 12288, 15 at 15360). Round 5: ONE batch
  // of 4, 8 or 16 slots covers a wave's whole range; slots past the end carry zero fragments (their MFMAs add +0: same sums bit for
  // bit as the ascending-k loop), so every launch of the denoise step waits for memory once. The launches are on the step's critical
  // path (tools/ab_engine_attr.py TL_SPLIT 4 1: 1.8 % of the step between one and four K-split slabs).
  int k = kbeg + wave * 32;
  const bf16x8 zero = {};
  auto batch = [&](auto n_) {
    constexpr int NS = decltype(n_)::value;
    bf16x8 af[NS], xf[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool in = k + u * 256 < kend;
      af[u] = in ? *(const bf16x8*)(ap + k + u * 256) : zero;
      xf[u] = in ? *(const bf16x8*)(xp + k + u * 256) : zero;
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if constexpr (F16) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, af[u]), __builtin_bit_cast(f16x8, xf[u]), acc, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u], xf[u], acc, 0, 0, 0);
    }
    k += NS * 256;
  };
  const int nsteps = k < kend ? (kend - k + 255) / 256 : 0;      // (wave-uniform)
  if (nsteps <= 4) batch(std::integral_constant<int, 4>{});
  else if (nsteps <= 8) batch(std::integral_constant<int, 8>{});
  else
    while (k < kend) batch(std::integral_constant<int, 16>{});
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 1; w < 8; ++w) {
      const f32x4 o = red[w][lane];
      acc[0] += o[0]; acc[1] += o[1]; acc[2] += o[2]; acc[3] += o[3];
    }
    // acc[j]: r = 4*kq + j, m = m0 + l15
    const int m = m0 + l15, r0 = 4 * kq;
    if (m < M && r0 < R) {
      float* tp = T + (size_t)m * ldt + r0;
      if (r0 + 4 <= R && (ldt & 3) == 0) *(f32x4*)tp = acc;
      else
        for (int j = 0; j < 4 && r0 + j < R; ++j) tp[j] = acc[j];
    }
  }
}

// Wide form, 16 < R <= 256 (adapters of rank > 4 behind a fused GEMM: up to four modules x rank 64): the same MFMA, operand roles and
// K-split slab contract, with blockIdx.z = a chunk of 64 r. A wave keeps up to four 16-r accumulators, so an X fragment is loaded
// once per 64 r, and the eight waves split the slab's K as above. Grid = (M / 16, n_split, R / 64): with the engine's four slabs
// that is one workgroup per CU at M = 1024, R = 64 (256 workgroups), and R / 64 times as many for the fused single-block adapters.
// Slabs are plain stores summed by the consumer in slab order; the waves' partial sums are added in wave order: no atomics.
template <bool F16>
__global__ __launch_bounds__(512) void lora_down_wide_kernel(const uint16_t* __restrict__ X, int ldx, const uint16_t* __restrict__ A,
                                                             float* __restrict__ T, int ldt, int M, int K, int R, int Ks, int split_stride) {
  __shared__ f32x4 red[8][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 16, rz0 = blockIdx.z * 64;
  const int nt = min(4, (R - rz0 + 15) / 16);                    // 16-r tiles of this chunk (workgroup-uniform)
  const int kbeg = blockIdx.y * Ks, kend = min(K, kbeg + Ks);
  T += (size_t)blockIdx.y * split_stride;
  const int l15 = lane & 15, kq = lane >> 4;
  const uint16_t* xp = X + (size_t)min(m0 + l15, M - 1) * ldx + kq * 8;
  const uint16_t* ap[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ap[t] = A + (size_t)min(rz0 + t * 16 + l15, R - 1) * K + kq * 8;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // as in lora_down_mfma_kernel: a batch's loads are all issued before its first MFMA, slots past the end carry zero fragments
  int k = kbeg + wave * 32;
  const bf16x8 zero = {};
  auto batch = [&](auto n_) {
    constexpr int NS = decltype(n_)::value;
    bf16x8 af[NS][4], xf[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool in = k + u * 256 < kend;
      xf[u] = in ? *(const bf16x8*)(xp + k + u * 256) : zero;
#pragma unroll
      for (int t = 0; t < 4; ++t) af[u][t] = (in && t < nt) ? *(const bf16x8*)(ap[t] + k + u * 256) : zero;
    }
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt) {
          if constexpr (F16) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, af[u][t]), __builtin_bit_cast(f16x8, xf[u]), acc[t], 0, 0, 0);
          else acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][t], xf[u], acc[t], 0, 0, 0);
        }
    k += NS * 256;
  };
  const int nsteps = k < kend ? (kend - k + 255) / 256 : 0;      // (wave-uniform)
  if (nsteps <= 4) batch(std::integral_constant<int, 4>{});
  else
    while (k < kend) batch(std::integral_constant<int, 8>{});
#pragma unroll
  for (int t = 0; t < 4; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave < nt) {                                               // wave t finishes tile t
    f32x4 s = red[0][wave][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) {
      const f32x4 o = red[w][wave][lane];
      s[0] += o[0]; s[1] += o[1]; s[2] += o[2]; s[3] += o[3];
    }
    // s[j]: r = rz0 + 16*wave + 4*kq + j, m = m0 + l15
    const int m = m0 + l15, r0 = rz0 + 16 * wave + 4 * kq;
    if (m < M && r0 < R) {
      float* tp = T + (size_t)m * ldt + r0;
      if (r0 + 4 <= R && (ldt & 3) == 0) *(f32x4*)tp = s;
      else
        for (int j = 0; j < 4 && r0 + j < R; ++j) tp[j] = s[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Skinny linear: Y[M<=16,N] fp32 = act_out(act_in(X[M,K]) . W[N,K]^T + bias). Weight-streaming (HBM bound):
// a wave owns 4 consecutive output columns, lanes split K in 16-B chunks, rows processed 4 at a time.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float silu(float x) { return x / (1.0f + __expf(-x)); }

__global__ __launch_bounds__(256) void linear_skinny_kernel(const float* __restrict__ X, int ldx, const uint16_t* __restrict__ W,
                                                            int ldw, const float* __restrict__ bias, float* __restrict__ Y,
                                                            int ldy, int M, int N, int K, int act_in, int act_out, int accumulate) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * 4;
  if (n0 >= N) return;
  const uint16_t* wr[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) wr[c] = W + (size_t)min(n0 + c, N - 1) * ldw;
  for (int mb = 0; mb < M; mb += 4) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      float wv[4][8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const u32x4 raw = *(const u32x4*)(wr[c] + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) { wv[c][2 * j] = __uint_as_float(raw[j] << 16); wv[c][2 * j + 1] = __uint_as_float(raw[j] & 0xffff0000u); }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (mb + i < M) {
          const float* xp = X + (size_t)(mb + i) * ldx + k;
          const f32x4 x0 = *(const f32x4*)xp, x1 = *(const f32x4*)(xp + 4);
          float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
          if (act_in == 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = silu(xv[j]);
          }
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][c] = fmaf(xv[j], wv[c][j], acc[i][c]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = wave_sum(acc[i][c]);
        if (lane == 0 && mb + i < M && n0 + c < N) {
          if (bias) s += bias[n0 + c];
          if (act_out == 1) s = silu(s);
          float* yp = Y + (size_t)(mb + i) * ldy + n0 + c;
          *yp = accumulate ? (*yp + s) : s;
        }
      }
  }
}

__global__ void timestep_embed_kernel(const float* __restrict__ t, float* __restrict__ out, int B, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim / 2;
  if (i >= B * half) return;
  const int b = i / half, j = i % half;
  const float f = expf(-9.210340371976184f * (float)j / (float)half);  // ln(10000)
  const float a = t[b] * f;
  out[(size_t)b * dim + j] = cosf(a);          // flip_sin_to_cos=True: [cos | sin]
  out[(size_t)b * dim + half + j] = sinf(a);
}

__global__ void convert_kernel(void* __restrict__ dst, int dst_bf16,const void* __restrict__ src, int src_bf16, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = src_bf16 ? bf16_to_f32(((const uint16_t*)src)[i]) : ((const float*)src)[i];
    if (dst_bf16 == 2) {          // fp16 (saturated): the operand image of an LX_OPERANDS_F16 GEMM
      float mx = 0.f;
      ((uint16_t*)dst)[i] = (uint16_t)(pack_f16x2_sat(v, 0.f, mx) & 0xffffu);
    } else if (dst_bf16) ((uint16_t*)dst)[i] = f32_to_bf16(v);
    else ((float*)dst)[i] = v;
  }
}

// ---- per-image adapter weights on the LoRA scratch: T_s[row, c] *= W[b, c % period] (lx_lora_scale_rows) ----------------------------
// One IEEE fp32 multiply per element. A work item is VEC columns of one row of one slab (VEC = 4: 16-byte accesses, taken when T, ldt,
// slab_stride allow it; a row's last chunk may be partial and goes by elements), items run slab-major over the segments' rows in launch
// order; grid-stride loop under a capped grid. No LDS: nothing is shared between items.
struct ScaleSegs {   // up to 3 row segments (token streams)
  int n;
  int row0[3], n_rows[3], rows_per_batch[3];
};

template <int VEC>
__global__ __launch_bounds__(256) void lora_scale_rows_kernel(float* __restrict__ T, int ldt, int R, int n_slab, int slab_stride, ScaleSegs segs,
                                                              int M, const float* __restrict__ W, int w_ld, int n_batches, int period) {
  const int cpr = (R + VEC - 1) / VEC;                       // chunks per row
  const size_t per_slab = (size_t)M * cpr, total = per_slab * n_slab;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int s = (int)(i / per_slab);
    const size_t in_slab = i - (size_t)s * per_slab;
    int rin = (int)(in_slab / cpr);
    const int c = (int)(in_slab - (size_t)rin * cpr) * VEC;
    int sg = 0;
    while (sg < segs.n - 1 && rin >= segs.n_rows[sg]) { rin -= segs.n_rows[sg]; ++sg; }
    const int b = (rin / segs.rows_per_batch[sg]) % n_batches;
    float* t = T + (size_t)s * slab_stride + (size_t)(segs.row0[sg] + rin) * ldt + c;
    const float* w = W + (size_t)b * w_ld;
    if (VEC == 4 && c + 4 <= R) {
      f32x4 v = *(const f32x4*)t;
      int p = c % period;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = v[j] * w[p];
        if (++p == period) p = 0;
      }
      *(f32x4*)t = v;
    } else {
      const int n = R - c < VEC ? R - c : VEC;
      for (int j = 0; j < n; ++j) t[j] = t[j] * w[(c + j) % period];
    }
  }
}

// ---- step-cache probe (lx_ln_modulate_delta) ----------------------------------------------------------------------------------------
// One wave per row, the three-pass row body of row_common.h: m = LN(x) * (1 + scale) + shift as ln_emit computes it, kept in fp32. While a
// chunk of m is at hand the lane reads the same chunk of P (the previous step's m), adds |m - P| and |P| to its two sums and stores m over
// it; lane sums run in chunk order, across lanes wave_sum's tree, lane 0 stores the row's pair. Nothing crosses a wave: no LDS, no atomics.
__global__ __launch_bounds__(256) void ln_modulate_delta_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ shift,
                                                                const float* __restrict__ scale, int mod_ld, float* __restrict__ P, int ldp,
                                                                int M, int D, int rows_per_batch, float eps, float* __restrict__ row_sums) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float* xr = X + (size_t)row * ldx;
  float mean, rstd;
  ln_row_stats(xr, D, lane, mean, rstd, eps);
  const int b = row / rows_per_batch;
  float* pr = P + (size_t)row * ldp;
  float s1 = 0.f, s2 = 0.f;
  ln_emit(xr, scale + (size_t)b * mod_ld, shift + (size_t)b * mod_ld, D, lane, mean, rstd, [&](int c, const float (&o)[4]) {
    const f32x4 p = *(const f32x4*)(pr + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s1 += fabsf(o[k] - p[k]);
      s2 += fabsf(p[k]);
    }
    *(f32x4*)(pr + c) = f32x4{o[0], o[1], o[2], o[3]};
  });
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) *(f32x2*)(row_sums + 2 * (size_t)row) = f32x2{s1, s2};
}

// The M row pairs added in row order, in double, by ONE wave: a lane loads the pair of row r0 + lane, the wave then walks its 64 lanes in
// order (v_readlane: every lane carries the same running sums). The order is fixed by construction, so the totals are the same bits from
// run to run; rows past M add +0.
__global__ __launch_bounds__(64) void row_pairs_total_kernel(const float* __restrict__ row_sums, int M, double* __restrict__ sums) {
  const int lane = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int r0 = 0; r0 < M; r0 += 64) {
    f32x2 v = {0.f, 0.f};
    if (r0 + lane < M) v = *(const f32x2*)(row_sums + 2 * (size_t)(r0 + lane));
    const float f0 = v[0], f1 = v[1];      // (plain floats first: __builtin_bit_cast of a vector-element lvalue reads element 0 for both)
    const int v0 = __builtin_bit_cast(int, f0), v1 = __builtin_bit_cast(int, f1);
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      a += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(v0, l));
      b += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(v1, l));
    }
  }
  if (lane == 0) {
    sums[0] = a;
    sums[1] = b;
  }
}

}  // namespace

// The five lx_ln_modulate* entry points. `name` is the one that was called: it reports the segment count and f16_ovf; everything else
// reports as lx_ln_modulate (the operands) or lx_ln_modulate_lora_segs (the adapter), whichever form was called.
static int ln_launch(const char* name, const float* X, int ldx, const lx_ln_seg* seg, int n_seg, int mod_ld, void* Y, int ldy, int D, float eps,
                     void* stream, const LnLora* lora = nullptr, bool f16 = false, int* f16_ovf = nullptr) {
  LX_CHECK_ARG(seg && n_seg >= 1 && n_seg <= 3, "%s: 1..3 segments", name);
  if (f16) LX_CHECK_ARG(((uintptr_t)f16_ovf & 3) == 0, "%s: f16_ovf must be 4-byte aligned", name);
  LnSegs segs;
  const int M = lx_ln_segs("lx_ln_modulate", seg, n_seg, segs);
  if (M < 0) return M;
  LX_CHECK_ARG(X && Y, "lx_ln_modulate: NULL operand");
  LX_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 16384, "lx_ln_modulate: D=%d must be a multiple of 4 and <= 16384", D);
  LX_CHECK_ARG(ldx % 4 == 0 && ldy % 4 == 0 && mod_ld % 4 == 0, "lx_ln_modulate: ldx/ldy/mod_ld must be multiples of 4");
  LX_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Y & 7) == 0, "lx_ln_modulate: misaligned operand");
  if (lora) {
    LX_CHECK_ARG(D == 3072 || D == 256, "lx_ln_modulate_lora_segs: the fused down-projection exists for D = 3072 and 256 (D=%d): use lx_lora_down", D);
    LX_CHECK_ARG(lora->A && lora->T && lora->R >= 1 && lora->R <= 16 && lora->ldt >= lora->R && lora->rows > 0 && lora->row0 >= 0,
                 "lx_ln_modulate_lora_segs: bad adapter arguments (R=%d)", lora->R);
    LX_CHECK_ARG(((uintptr_t)lora->A & 15) == 0, "lx_ln_modulate_lora_segs: Adown must be 16-byte aligned");
  }
  const LnLora lo = lora ? *lora : LnLora{};
  auto launch = [&](auto kernel, auto... tail) {
    hipLaunchKernelGGL(kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, ldx, segs, mod_ld, (uint16_t*)Y, ldy, M, D, eps, tail...);
  };
  auto dispatch = [&](auto lm, auto h) {      // (LM, F16) -> the kernel for this D
    constexpr bool LM = decltype(lm)::value, F16 = decltype(h)::value;
    if (D == 3072) launch(ln_modulate_kernel<12, LM, F16>, lo, f16_ovf);
    else if (D == 256) launch(ln_modulate_kernel<1, LM, F16>, lo, f16_ovf);
    else if constexpr (!LM) launch(ln_modulate_generic<F16>, f16_ovf);
  };
  if (lora && f16) dispatch(std::true_type{}, std::true_type{});
  else if (lora) dispatch(std::true_type{}, std::false_type{});
  else if (f16) dispatch(std::false_type{}, std::true_type{});
  else dispatch(std::false_type{}, std::false_type{});
  LX_LAUNCH_CHECK(lora ? "lx_ln_modulate_lora_segs" : f16 ? "lx_ln_modulate_f16_segs" : "lx_ln_modulate");
  return LX_OK;
}

extern "C" int lx_ln_modulate(const float* X, int ldx, const float* shift, const float* scale, int mod_ld, void* Y, int ldy,
                              int M, int D, int rows_per_batch, float eps, void* stream) {
  LX_CHECK_ARG(M > 0, "lx_ln_modulate: M must be > 0");
  const lx_ln_seg one = {0, M, rows_per_batch, 0, shift, scale};
  return ln_launch("lx_ln_modulate", X, ldx, &one, 1, mod_ld, Y, ldy, D, eps, stream);
}

extern "C" int lx_ln_modulate_segs(const float* X, int ldx, const lx_ln_seg* seg, int n_seg, int mod_ld, void* Y, int ldy, int D,
                                   float eps, void* stream) {
  return ln_launch("lx_ln_modulate_segs", X, ldx, seg, n_seg, mod_ld, Y, ldy, D, eps, stream);
}

extern "C" int lx_ln_modulate_f16_segs(const float* X, int ldx, const lx_ln_seg* seg, int n_seg, int mod_ld, void* Y, int ldy, int D,
                                       float eps, int32_t* f16_ovf, void* stream) {
  return ln_launch("lx_ln_modulate_f16_segs", X, ldx, seg, n_seg, mod_ld, Y, ldy, D, eps, stream, nullptr, true, (int*)f16_ovf);
}

extern "C" int lx_ln_modulate_lora_f16_segs(const float* X, int ldx, const lx_ln_seg* seg, int n_seg, int mod_ld, void* Y, int ldy, int D,
                                            float eps, const void* Adown, int R, float* T, int ldt, int lora_row0, int lora_rows,
                                            int32_t* f16_ovf, void* stream) {
  const LnLora lo{(const uint16_t*)Adown, T, R, ldt, lora_row0, lora_rows};
  return ln_launch("lx_ln_modulate_lora_f16_segs", X, ldx, seg, n_seg, mod_ld, Y, ldy, D, eps, stream, &lo, true, (int*)f16_ovf);
}

extern "C" int lx_ln_modulate_lora_segs(const float* X, int ldx, const lx_ln_seg* seg, int n_seg, int mod_ld, void* Y, int ldy, int D,
                                        float eps, const void* Adown, int R, float* T, int ldt, int lora_row0, int lora_rows, void* stream) {
  const LnLora lo{(const uint16_t*)Adown, T, R, ldt, lora_row0, lora_rows};
  return ln_launch("lx_ln_modulate_lora_segs", X, ldx, seg, n_seg, mod_ld, Y, ldy, D, eps, stream, &lo);
}

// lx_qkv_prep and its two _segs forms: all report as lx_qkv_prep, the segment count as lx_qkv_prep_segs. vt_pos0 is looked at only when
// a V^T image is written.
static int qkv_launch(void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg, int n_batches, int H, float eps,
                      void* VT, int vt_ld, void* stream, bool in_f16 = false) {
  LX_CHECK_ARG(seg && n_seg >= 1 && n_seg <= 3, "lx_qkv_prep_segs: 1..3 segments");
  LX_CHECK_ARG(QKV && n_batches > 0 && H > 0, "lx_qkv_prep: bad arguments");
  LX_CHECK_ARG(ld % 8 == 0 && q_col % 8 == 0 && k_col % 8 == 0 && v_col % 8 == 0, "lx_qkv_prep: ld and column offsets must be multiples of 8");
  if (VT) LX_CHECK_ARG(vt_ld % 64 == 0, "lx_qkv_prep: vt_ld must be a multiple of 64");
  QkvSegs segs;
  const int t = lx_qkv_segs("lx_qkv_prep", seg, n_seg, VT ? LX_VT_POS0_MULT64 : LX_VT_POS0_ANY, segs);
  if (t < 0) return t;
  bool fast = true;
  for (int i = 0; i < segs.n; ++i) fast = fast && segs.wq[i] && segs.wk[i] && segs.cos_tab[i];
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(t, H, n_batches), dim3(256), 0, (hipStream_t)stream, (uint16_t*)QKV, ld, q_col, k_col, v_col, segs, eps,
                       (uint16_t*)VT, vt_ld, H, (uint16_t*)nullptr, 0, 0);
  };
  if (in_f16) launch(qkv_prep_kernel<false, true>);
  else if (fast) launch(qkv_prep_kernel<true>);
  else launch(qkv_prep_kernel<false>);
  LX_LAUNCH_CHECK("lx_qkv_prep");
  return LX_OK;
}

extern "C" int lx_qkv_prep(void* QKV, int ld, int q_col, int k_col, int v_col, int row0, int n_rows, int rows_per_batch, int H,
                           const float* wq, const float* wk, float eps, const float* cos_tab, const float* sin_tab, void* VT,
                           int vt_ld, int vt_pos0, void* stream) {
  LX_CHECK_ARG(n_rows > 0 && rows_per_batch > 0 && n_rows % rows_per_batch == 0, "lx_qkv_prep: n_rows=%d must be a multiple of rows_per_batch=%d", n_rows, rows_per_batch);
  const lx_qkv_seg one = {row0, rows_per_batch, vt_pos0, 0, wq, wk, cos_tab, sin_tab};
  return qkv_launch(QKV, ld, q_col, k_col, v_col, &one, 1, n_rows / rows_per_batch, H, eps, VT, vt_ld, stream);
}

extern "C" int lx_qkv_prep_segs(void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg, int n_batches,
                                int H, float eps, void* VT, int vt_ld, void* stream) {
  return qkv_launch(QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, VT, vt_ld, stream);
}

extern "C" int lx_qkv_prep_f16in_segs(void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg, int n_batches,
                                      int H, float eps, void* VT, int vt_ld, void* stream) {
  return qkv_launch(QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, VT, vt_ld, stream, true);
}

// lx_qkv_prep_kv_segs / lx_qkv_prep_kv_f16in_segs: the pass above with the keys in an image of their own (qkv_prep_kernel<.., KIMG>). A launch
// over some segments into images that keep other segments' entries: nothing may land outside the rows and the 64-slot tiles of the segments
// it is given, so every tile has to end inside vt_ld and the key columns inside ldk2 (checked here, before the launch).
static int qkv_kv_launch(const char* fn, bool in_f16, void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg,
                         int n_batches, int H, float eps, void* K2, int ldk2, int k2_col, void* VT, int vt_ld, void* stream) {
  LX_CHECK_ARG(seg && n_seg >= 1 && n_seg <= 3, "%s: 1..3 segments", fn);
  LX_CHECK_ARG(QKV && K2 && VT && n_batches > 0 && H > 0, "%s: bad arguments", fn);
  LX_CHECK_ARG(ld % 8 == 0 && q_col % 8 == 0 && k_col % 8 == 0 && v_col % 8 == 0 && ((uintptr_t)QKV & 15) == 0,
               "%s: ld and column offsets must be multiples of 8, QKV 16-byte aligned", fn);
  LX_CHECK_ARG(ldk2 % 8 == 0 && k2_col % 8 == 0 && k2_col >= 0 && ldk2 >= k2_col + H * 128 && ((uintptr_t)K2 & 15) == 0,
               "%s: ldk2=%d / k2_col=%d must be multiples of 8 with k2_col + H*128 <= ldk2, K2 16-byte aligned", fn, ldk2, k2_col);
  LX_CHECK_ARG(vt_ld % 64 == 0 && ((uintptr_t)VT & 15) == 0, "%s: vt_ld must be a multiple of 64, VT 16-byte aligned", fn);
  QkvSegs segs;
  const int t = lx_qkv_segs(fn, seg, n_seg, LX_VT_POS0_MULT64_NONNEG, segs);
  if (t < 0) return t;
  for (int i = 0; i < n_seg; ++i) {
    const long long vt_end = (long long)seg[i].vt_pos0 + (seg[i].rows_per_batch + 63) / 64 * 64;
    LX_CHECK_ARG(vt_end <= vt_ld, "%s: segment %d's V^T tiles end at %lld > vt_ld=%d", fn, i, vt_end, vt_ld);
  }
  bool fast = true;
  for (int i = 0; i < segs.n; ++i) fast = fast && segs.wq[i] && segs.wk[i] && segs.cos_tab[i];
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(t, H, n_batches), dim3(256), 0, (hipStream_t)stream, (uint16_t*)QKV, ld, q_col, k_col, v_col, segs, eps,
                       (uint16_t*)VT, vt_ld, H, (uint16_t*)K2, ldk2, k2_col);
  };
  if (in_f16) launch(qkv_prep_kernel<false, true, true>);
  else if (fast) launch(qkv_prep_kernel<true, false, true>);
  else launch(qkv_prep_kernel<false, false, true>);
  LX_LAUNCH_CHECK(fn);
  return LX_OK;
}

extern "C" int lx_qkv_prep_kv_segs(void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg, int n_batches,
                                   int H, float eps, void* K2, int ldk2, int k2_col, void* VT, int vt_ld, void* stream) {
  return qkv_kv_launch("lx_qkv_prep_kv_segs", false, QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, K2, ldk2, k2_col, VT, vt_ld, stream);
}

extern "C" int lx_qkv_prep_kv_f16in_segs(void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg, int n_batches,
                                         int H, float eps, void* K2, int ldk2, int k2_col, void* VT, int vt_ld, void* stream) {
  return qkv_kv_launch("lx_qkv_prep_kv_f16in_segs", true, QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, K2, ldk2, k2_col, VT, vt_ld,
                       stream);
}

static int qkv_fp8_segs_launch(bool in_f16, const void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg,
                               int n_batches, int H, float eps, void* Q8, void* K8, int ld8, void* VT8, int vt8_ld,
                               float q_scale, float k_scale, float v_scale, void* stream) {
  LX_CHECK_ARG(seg && n_seg >= 1 && n_seg <= 3, "lx_qkv_prep_fp8_segs: 1..3 segments");
  LX_CHECK_ARG(QKV && Q8 && K8 && VT8 && n_batches > 0 && H > 0, "lx_qkv_prep_fp8_segs: bad arguments");
  LX_CHECK_ARG(ld % 8 == 0 && q_col % 8 == 0 && k_col % 8 == 0 && v_col % 8 == 0, "lx_qkv_prep_fp8_segs: ld and column offsets must be multiples of 8");
  LX_CHECK_ARG(ld8 % 16 == 0 && vt8_ld % 64 == 0, "lx_qkv_prep_fp8_segs: ld8 %% 16 and vt8_ld %% 64 required");
  LX_CHECK_ARG(q_scale > 0.f && k_scale > 0.f && v_scale > 0.f, "lx_qkv_prep_fp8_segs: scales must be positive");
  QkvSegs segs;
  const int t = lx_qkv_segs("lx_qkv_prep_fp8_segs", seg, n_seg, LX_VT_POS0_MULT64, segs);
  if (t < 0) return t;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(t, H, n_batches), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV, ld, q_col, k_col, v_col, segs, eps,
                       (uint8_t*)Q8, (uint8_t*)K8, ld8, (uint8_t*)VT8, vt8_ld, H, q_scale, k_scale, v_scale);
  };
  if (in_f16) launch(qkv_prep_fp8_kernel<true>);
  else launch(qkv_prep_fp8_kernel<false>);
  LX_LAUNCH_CHECK("lx_qkv_prep_fp8_segs");
  return LX_OK;
}

extern "C" int lx_qkv_prep_fp8_segs(const void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg,
                                    int n_batches, int H, float eps, void* Q8, void* K8, int ld8, void* VT8, int vt8_ld,
                                    float q_scale, float k_scale, float v_scale, void* stream) {
  return qkv_fp8_segs_launch(false, QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, Q8, K8, ld8, VT8, vt8_ld, q_scale, k_scale, v_scale,
                             stream);
}

extern "C" int lx_qkv_prep_fp8_f16in_segs(const void* QKV, int ld, int q_col, int k_col, int v_col, const lx_qkv_seg* seg, int n_seg,
                                          int n_batches, int H, float eps, void* Q8, void* K8, int ld8, void* VT8, int vt8_ld,
                                          float q_scale, float k_scale, float v_scale, void* stream) {
  return qkv_fp8_segs_launch(true, QKV, ld, q_col, k_col, v_col, seg, n_seg, n_batches, H, eps, Q8, K8, ld8, VT8, vt8_ld, q_scale, k_scale, v_scale,
                             stream);
}

static int lora_down_launch(const char* name, bool f16, const void* X, int ldx, const void* Adown, float* T, int ldt, int M, int K, int R, int n_split,
                            int split_stride, void* stream) {
  LX_CHECK_ARG(X && Adown && T && M > 0, "%s: NULL operand", name);
  LX_CHECK_ARG(R >= 1 && R <= 256, "%s: R=%d must be in [1,256]", name, R);
  LX_CHECK_ARG(K % 32 == 0 && ldx % 8 == 0 && ldt >= R, "%s: K %% 32, ldx %% 8 and ldt >= R required (K=%d)", name, K);
  LX_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Adown & 15) == 0 && ((uintptr_t)T & 15) == 0, "%s: operands must be 16-byte aligned", name);
  LX_CHECK_ARG(n_split >= 1 && n_split <= 16 && (n_split == 1 || split_stride >= (M - 1) * ldt + R) && split_stride % 4 == 0,
               "%s: bad n_split=%d / split_stride=%d", name, n_split, split_stride);
  const int Ks = ((K / 32 + n_split - 1) / n_split) * 32;
  if (R > 16) {                      // the wide form: 64 r per workgroup
    const dim3 grid((M + 15) / 16, n_split, (R + 63) / 64);
    if (f16) hipLaunchKernelGGL(lora_down_wide_kernel<true>, grid, dim3(512), 0, (hipStream_t)stream, (const uint16_t*)X, ldx, (const uint16_t*)Adown, T, ldt, M, K, R, Ks, split_stride);
    else hipLaunchKernelGGL(lora_down_wide_kernel<false>, grid, dim3(512), 0, (hipStream_t)stream, (const uint16_t*)X, ldx, (const uint16_t*)Adown, T, ldt, M, K, R, Ks, split_stride);
    LX_LAUNCH_CHECK(name);
    return LX_OK;
  }
  LoraTerms lt = {};
  lt.X[0] = (const uint16_t*)X; lt.A[0] = (const uint16_t*)Adown; lt.ldx[0] = ldx; lt.n = 0;
  if (f16) hipLaunchKernelGGL(lora_down_mfma_kernel<true>, dim3((M + 15) / 16, n_split), dim3(512), 0, (hipStream_t)stream, lt, T, ldt, M, K, R, Ks, split_stride);
  else hipLaunchKernelGGL(lora_down_mfma_kernel<false>, dim3((M + 15) / 16, n_split), dim3(512), 0, (hipStream_t)stream, lt, T, ldt, M, K, R, Ks, split_stride);
  LX_LAUNCH_CHECK(name);
  return LX_OK;
}

extern "C" int lx_lora_down(const void* X, int ldx, const void* Adown, float* T, int ldt, int M, int K, int R, int n_split,
                            int split_stride, void* stream) {
  return lora_down_launch("lx_lora_down", false, X, ldx, Adown, T, ldt, M, K, R, n_split, split_stride, stream);
}

extern "C" int lx_lora_down_f16(const void* X, int ldx, const void* Adown, float* T, int ldt, int M, int K, int R, int n_split,
                                int split_stride, void* stream) {
  return lora_down_launch("lx_lora_down_f16", true, X, ldx, Adown, T, ldt, M, K, R, n_split, split_stride, stream);
}

extern "C" int lx_lora_down_terms(const void* const* X, const int* ldx, const void* const* Adown, int n_terms, float* T, int ldt, int M, int K,
                                  int R, int slab_stride, void* stream) {
  LX_CHECK_ARG(X && ldx && Adown && T && M > 0 && n_terms >= 1 && n_terms <= 4, "lx_lora_down_terms: bad arguments (1..4 terms)");
  LX_CHECK_ARG(R >= 1 && R <= 16 && K % 32 == 0 && ldt >= R && ((uintptr_t)T & 15) == 0, "lx_lora_down_terms: R in [1,16], K %% 32, ldt >= R, T 16-byte aligned required");
  LX_CHECK_ARG((n_terms == 1 || slab_stride >= (M - 1) * ldt + R) && slab_stride % 4 == 0, "lx_lora_down_terms: bad slab_stride=%d", slab_stride);
  LoraTerms lt = {};
  lt.n = n_terms;
  for (int i = 0; i < n_terms; ++i) {
    LX_CHECK_ARG(X[i] && Adown[i] && ldx[i] % 8 == 0 && ((uintptr_t)X[i] & 15) == 0 && ((uintptr_t)Adown[i] & 15) == 0, "lx_lora_down_terms: term %d: NULL / misaligned operand or ldx %% 8", i);
    lt.X[i] = (const uint16_t*)X[i]; lt.A[i] = (const uint16_t*)Adown[i]; lt.ldx[i] = ldx[i];
  }
  hipLaunchKernelGGL(lora_down_mfma_kernel<false>, dim3((M + 15) / 16, n_terms), dim3(512), 0, (hipStream_t)stream, lt, T, ldt, M, K, R, K, slab_stride);
  LX_LAUNCH_CHECK("lx_lora_down_terms");
  return LX_OK;
}

extern "C" int lx_lora_scale_rows(float* T, int ldt, int R, int n_slab, int slab_stride, const lx_rowscale_seg* seg, int n_seg,
                                  const float* W, int w_ld, int n_batches, int period, void* stream) {
  LX_CHECK_ARG(T && W && seg, "lx_lora_scale_rows: NULL operand");
  LX_CHECK_ARG(R >= 1 && R <= 16384, "lx_lora_scale_rows: R=%d must be in [1,16384]", R);
  LX_CHECK_ARG(period >= 1 && n_batches >= 1 && n_slab >= 1, "lx_lora_scale_rows: period=%d, n_batches=%d and n_slab=%d must be >= 1", period,
               n_batches, n_slab);
  LX_CHECK_ARG(n_seg >= 1 && n_seg <= 3, "lx_lora_scale_rows: 1..3 segments");
  LX_CHECK_ARG(w_ld >= (period < R ? period : R), "lx_lora_scale_rows: w_ld=%d must be >= min(period, R)", w_ld);
  LX_CHECK_ARG(ldt >= R, "lx_lora_scale_rows: ldt=%d must be >= R=%d", ldt, R);
  LX_CHECK_ARG(n_slab == 1 || slab_stride > 0, "lx_lora_scale_rows: bad slab_stride=%d", slab_stride);
  LX_CHECK_ARG((((uintptr_t)T | (uintptr_t)W) & 3) == 0, "lx_lora_scale_rows: operands must be 4-byte aligned");
  ScaleSegs segs = {};
  segs.n = n_seg;
  long long M = 0;
  for (int i = 0; i < n_seg; ++i) {
    LX_CHECK_ARG(seg[i].row0 >= 0 && seg[i].n_rows > 0 && seg[i].rows_per_batch >= 1, "lx_lora_scale_rows: bad segment %d", i);
    segs.row0[i] = seg[i].row0; segs.n_rows[i] = seg[i].n_rows; segs.rows_per_batch[i] = seg[i].rows_per_batch;
    M += seg[i].n_rows;
  }
  LX_CHECK_ARG(M <= 0x7fffffffLL, "lx_lora_scale_rows: too many rows");
  // 16-byte accesses where every chunk of every row of every slab starts on a 16-byte boundary; elements otherwise (ldt = 22)
  const bool vec = ((uintptr_t)T & 15) == 0 && ldt % 4 == 0 && (n_slab == 1 || slab_stride % 4 == 0);
  const size_t items = (size_t)M * (size_t)(vec ? (R + 3) / 4 : R) * (size_t)n_slab;
  const int grid = (int)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);
  if (vec) hipLaunchKernelGGL(lora_scale_rows_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, T, ldt, R, n_slab, slab_stride, segs, (int)M, W, w_ld, n_batches, period);
  else hipLaunchKernelGGL(lora_scale_rows_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, T, ldt, R, n_slab, slab_stride, segs, (int)M, W, w_ld, n_batches, period);
  LX_LAUNCH_CHECK("lx_lora_scale_rows");
  return LX_OK;
}

extern "C" int lx_linear_skinny(const float* X, int ldx, const void* W, int ldw, const float* bias, float* Y, int ldy, int M, int N,
                                int K, int act_in, int act_out, int accumulate, void* stream) {
  LX_CHECK_ARG(X && W && Y, "lx_linear_skinny: NULL operand");
  LX_CHECK_ARG(M >= 1 && M <= 65536, "lx_linear_skinny: M=%d must be in [1,65536]", M);
  LX_CHECK_ARG(K % 8 == 0 && ldw % 8 == 0 && ldx % 4 == 0, "lx_linear_skinny: K %% 8, ldw %% 8, ldx %% 4 required (K=%d)", K);
  const dim3 grid((N + 15) / 16), block(256);
  hipLaunchKernelGGL(linear_skinny_kernel, grid, block, 0, (hipStream_t)stream, X, ldx, (const uint16_t*)W, ldw, bias, Y, ldy, M, N,
                     K, act_in, act_out, accumulate);
  LX_LAUNCH_CHECK("lx_linear_skinny");
  return LX_OK;
}

extern "C" int lx_timestep_embed(const float* t, float* out, int B, int dim, void* stream) {
  LX_CHECK_ARG(t && out && B > 0 && dim > 0 && dim % 2 == 0, "lx_timestep_embed: bad arguments");
  const int n = B * dim / 2;
  hipLaunchKernelGGL(timestep_embed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, out, B, dim);
  LX_LAUNCH_CHECK("lx_timestep_embed");
  return LX_OK;
}

extern "C" int lx_ln_modulate_delta(const float* X, int ldx, const float* shift, const float* scale, int mod_ld, float* P, int ldp, int M, int D,
                                    int rows_per_batch, float eps, float* row_sums, double* sums, void* stream) {
  LX_CHECK_ARG(X && shift && scale && P && row_sums && sums, "lx_ln_modulate_delta: NULL operand");
  LX_CHECK_ARG(M > 0 && rows_per_batch > 0, "lx_ln_modulate_delta: M=%d and rows_per_batch=%d must be > 0", M, rows_per_batch);
  LX_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 16384, "lx_ln_modulate_delta: D=%d must be a multiple of 4 and <= 16384", D);
  LX_CHECK_ARG(ldx % 4 == 0 && ldp % 4 == 0 && mod_ld % 4 == 0 && ldx >= D && ldp >= D && mod_ld >= D,
               "lx_ln_modulate_delta: ldx/ldp/mod_ld must be multiples of 4 and >= D");
  LX_CHECK_ARG((((uintptr_t)X | (uintptr_t)shift | (uintptr_t)scale | (uintptr_t)P) & 15) == 0 &&
                   (((uintptr_t)row_sums | (uintptr_t)sums) & 7) == 0, "lx_ln_modulate_delta: misaligned operand");
  const size_t xbytes = ((size_t)(M - 1) * ldx + D) * sizeof(float), pbytes = ((size_t)(M - 1) * ldp + D) * sizeof(float);
  LX_CHECK_ARG(!byte_ranges_overlap(X, xbytes, P, pbytes), "lx_ln_modulate_delta: P may not overlap X");
  hipLaunchKernelGGL(ln_modulate_delta_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, X, ldx, shift, scale, mod_ld, P, ldp, M, D,
                     rows_per_batch, eps, row_sums);
  hipLaunchKernelGGL(row_pairs_total_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)row_sums, M, sums);
  LX_LAUNCH_CHECK("lx_ln_modulate_delta");
  return LX_OK;
}

extern "C" int lx_convert(void* dst, int dst_bf16, const void* src, int src_bf16, size_t n, void* stream) {
  LX_CHECK_ARG(dst && src, "lx_convert: NULL operand");
  if (n == 0) return LX_OK;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(convert_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dst, dst_bf16, src, src_bf16, n);
  LX_LAUNCH_CHECK("lx_convert");
  return LX_OK;
}

// ------------------------------------------------------------------------------------------------------
// RoPE tables (diffusers FluxPosEmbed / get_1d_rotary_pos_embed, transformer.py:130-134): fp64 frequencies,
// repeat-interleaved real layout, stored fp32. One thread per (position, rotary pair).
// ------------------------------------------------------------------------------------------------------
namespace {
__global__ void rope_table_kernel(const float* __restrict__ ids, int n_axes, int a0, int a1, int a2, double theta,
                                  float* __restrict__ cos_t, float* __restrict__ sin_t, int L) {
  const int dims[3] = {a0, a1, a2};
  const int total = a0 + a1 + a2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L * (total / 2)) return;
  const int p = i / (total / 2);
  int j = i % (total / 2), axis = 0, off = 0;
  while (axis < n_axes - 1 && j >= dims[axis] / 2) { j -= dims[axis] / 2; off += dims[axis]; ++axis; }
  const double freq = 1.0 / pow(theta, (double)(2 * j) / (double)dims[axis]);
  const double ang = (double)ids[(size_t)p * n_axes + axis] * freq;
  const float c = (float)cos(ang), s = (float)sin(ang);
  const size_t o = (size_t)p * total + off + 2 * j;
  cos_t[o] = c; cos_t[o + 1] = c;
  sin_t[o] = s; sin_t[o + 1] = s;
}
}  // namespace

extern "C" int lx_rope_table(const float* ids, int L, int a0, int a1, int a2, double theta, float* cos_t, float* sin_t, void* stream) {
  LX_CHECK_ARG(ids && cos_t && sin_t && L > 0, "lx_rope_table: bad arguments");
  LX_CHECK_ARG(a0 > 0 && a1 > 0 && a2 > 0 && a0 % 2 == 0 && a1 % 2 == 0 && a2 % 2 == 0, "lx_rope_table: axes dims must be positive and even");
  const int n = L * (a0 + a1 + a2) / 2;
  hipLaunchKernelGGL(rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, 3, a0, a1, a2, theta, cos_t, sin_t, L);
  LX_LAUNCH_CHECK("lx_rope_table");
  return LX_OK;
}
