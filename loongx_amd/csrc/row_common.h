// row_common.h -- the row bodies the operand modes share (rowops.hip: bf16 / fp16, fp8.hip and rowops.hip: e4m3, precise.hip: fp32 and
// bf16 hi/lo pairs): per-head RMSNorm(128) + interleaved-pair RoPE of the separate q/k/v pass, and the generic three-pass AdaLN
// LayerNorm. A kernel supplies how values are loaded and stored; the arithmetic, in one fixed order of operations, is here.
#pragma once
#include "common.h"

namespace {

// ---- q/k/v pass: workgroup = 64 positions x 1 head x 1 batch; 16 lanes own one (row, head) vector of 128 (8 elements = 4 rotary pairs each)
struct QkvTile {
  int sg, p0, row0, rows_per_batch;   // segment, first position of the tile within a batch, the segment's first row and positions per batch
  int h, b, sub, rloc;                // head, batch, 8-element chunk of the head vector, row within a 16-row pass
  __device__ __forceinline__ size_t rbase() const { return (size_t)row0 + (size_t)b * rows_per_batch; }   // row of position 0 of this batch
};
// bid / tid: the kernel's blockIdx / threadIdx. (Taken as they are and read member by member, result by reference, rbase() left to the
// caller: with a dim3 copy, a struct return or rbase computed here, hipcc orders the FAST body of qkv_prep_kernel differently.)
template <class Bid, class Tid>
__device__ __forceinline__ void qkv_tile(const QkvSegs& segs, const Bid& bid, const Tid& tid, QkvTile& t) {
  t.sg = 0;
  while (t.sg < segs.n - 1 && (int)bid.x >= segs.tile0[t.sg + 1]) ++t.sg;
  t.p0 = ((int)bid.x - segs.tile0[t.sg]) * 64;
  t.row0 = segs.row0[t.sg];
  t.rows_per_batch = segs.rows_per_batch[t.sg];
  t.h = bid.y;
  t.b = bid.z;
  t.sub = tid.x & 15;
  t.rloc = tid.x >> 4;
}

// the lane's 8 cos and 8 sin values of position p (tables [positions, 128] fp32, repeat-interleaved: entries 2i and 2i+1 are equal).
// No tables, or a row past the end: the identity rotation.
__device__ __forceinline__ void rope_rows(const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, int p, int sub, bool valid,
                                          f32x4& c0, f32x4& c1, f32x4& s0, f32x4& s1) {
  c0 = f32x4{1.f, 1.f, 1.f, 1.f}; c1 = c0;
  s0 = f32x4{0.f, 0.f, 0.f, 0.f}; s1 = s0;
  if (cos_tab && valid) {
    const float* ct = cos_tab + (size_t)p * 128 + sub * 8;
    const float* st = sin_tab + (size_t)p * 128 + sub * 8;
    c0 = *(const f32x4*)ct; c1 = *(const f32x4*)(ct + 4);
    s0 = *(const f32x4*)st; s1 = *(const f32x4*)(st + 4);
  }
}

// RMSNorm over the head's 128 values (wn != nullptr: the lane's weights are wn[sub*8 .. +8)), then RoPE, on the lane's 8 values (diffusers
// RMSNorm / apply_rotary_emb, block.py:60-99). Everything in fp32 whatever the storage format: x * rsqrt(mean(x^2) + eps) * w, eps INSIDE
// the root; the sum of squares is the lane's 8 in index order, then the xor-shuffle tree over the row's 16 lanes. Rotation of the
// interleaved pairs (2i, 2i+1): out = x*cos + rot*sin with rot = (-x_odd, x_even). x is overwritten by the normalised values.
// (The FAST body of qkv_prep_kernel and the LX_EPI_QKV epilogues of gemm8.h / gemm4.h hold copies of this arithmetic in their own layouts.)
__device__ __forceinline__ void rms_rope8(float (&x)[8], const float* __restrict__ wn, int sub, float eps, const f32x4 c0, const f32x4 c1,
                                          const f32x4 s0, const f32x4 s1, float (&y)[8]) {
  if (wn) {
    // The order is written out, not left to contraction: x0^2 fused onto the rounded x1^2, the other six products rounded before they are
    // added. That is what hipcc made of every copy of this body that reads fp32, so their bits are kept (on 16-bit inputs every product
    // is exact and any order of fusing gives the same sum); left alone, which of the eight it fuses depends on how the vectoriser pairs
    // them, and that on the code around the call.
    float ss;
    {
#pragma clang fp contract(off)
      ss = __builtin_fmaf(x[0], x[0], x[1] * x[1]);
#pragma unroll
      for (int i = 2; i < 8; ++i) ss += x[i] * x[i];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float r = rsqrtf(ss * (1.0f / 128.0f) + eps);   // one fma in every kernel: a product with a single use, an add, always fused
    const f32x4 w0 = *(const f32x4*)(wn + sub * 8), w1 = *(const f32x4*)(wn + sub * 8 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = x[i] * r * w0[i]; x[4 + i] = x[4 + i] * r * w1[i]; }
  }
  // The rotation stays left to contraction, because no one written-out form keeps every kernel's bits: the copies this body replaced
  // already disagreed. hipcc fuses x*cos onto the rounded x'*sin in the bf16, fp32 and pair kernels and rounds both products in the
  // e4m3 kernels (where y * scale follows), and does the same with this body inlined. A change of compiler is checked by hashing the
  // kernels' outputs against the previous build's.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float ce = i < 2 ? c0[2 * i] : c1[2 * i - 4], co = i < 2 ? c0[2 * i + 1] : c1[2 * i - 3];
    const float se = i < 2 ? s0[2 * i] : s1[2 * i - 4], so = i < 2 ? s0[2 * i + 1] : s1[2 * i - 3];
    y[2 * i] = x[2 * i] * ce - x[2 * i + 1] * se;
    y[2 * i + 1] = x[2 * i + 1] * co + x[2 * i] * so;
  }
}

// The general pass loop: four 16-row passes, each q then k, then the lane's chunk of V into the kernel's transpose buffer. IO is the
// kernel's storage format:
//   io.row(r)                    go to global row r (row 0 of the batch stands in for positions past the end: !valid below). Once per pass,
//                                unconditional: the row's address arithmetic stays out of the `valid` branches
//   io.load8(which, valid, x)    x[8] <- the lane's chunk of q (which = 0) or k (1); zeros when !valid
//   io.store8(which, valid, y)   the rotated chunk to wherever the format keeps it; nothing when !valid
//   io.stash_v(pass, valid)      V chunk -> LDS row pass * 16 + rloc for the V^T transpose after the loop (zeros when !valid)
template <class IO>
__device__ __forceinline__ void qkv_prep_rows(const QkvSegs& segs, const QkvTile& t, float eps, IO& io) {
  const float* __restrict__ wq = segs.wq[t.sg];
  const float* __restrict__ wk = segs.wk[t.sg];
  const float* __restrict__ cos_tab = segs.cos_tab[t.sg];
  const float* __restrict__ sin_tab = segs.sin_tab[t.sg];
  const size_t rbase = t.rbase();
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int p = t.p0 + pass * 16 + t.rloc;
    const bool valid = p < t.rows_per_batch;
    io.row(rbase + (valid ? p : 0));
    f32x4 c0, c1, s0, s1;
    rope_rows(cos_tab, sin_tab, p, t.sub, valid, c0, c1, s0, s1);
#pragma unroll
    for (int which = 0; which < 2; ++which) {   // 0: q, 1: k
      float x[8], y[8];
      io.load8(which, valid, x);
      rms_rope8(x, which ? wk : wq, t.sub, eps, c0, c1, s0, s1, y);
      io.store8(which, valid, y);
    }
    io.stash_v(pass, valid);
  }
}

// ---- generic AdaLN LayerNorm (no affine) + modulation, fp32 in: one wave per row, three passes over the (L2-resident) row, D % 4 == 0 ----
// launch-order row -> segment sg, row in segment rin and the physical row (in `row`); false: the wave has no row
__device__ __forceinline__ bool ln_row(const LnSegs& segs, int M, int& row, int& rin, int& sg) {
  if (row >= M) return false;
  int acc_rows = 0;
  sg = 0;
  while (sg < segs.n - 1 && row >= acc_rows + segs.n_rows[sg]) { acc_rows += segs.n_rows[sg]; ++sg; }
  rin = row - acc_rows;
  row = segs.row0[sg] + rin;
  return true;
}
// mean, then the variance about it in a second pass (not E[x^2] - mean^2: cancellation); eps inside the root. Lane sums in chunk order,
// each chunk as (v0+v1)+(v2+v3); across lanes wave_sum's tree.
__device__ __forceinline__ void ln_row_stats(const float* __restrict__ xr, int D, int lane, float& mean, float& rstd, float eps) {
  float s = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) q += (v[k] - mean) * (v[k] - mean);
  }
  rstd = rsqrtf(wave_sum(q) / (float)D + eps);
}
// third pass: o = (x - mean) * rstd * (1 + scale) + shift with the modulation rows sc / sh of the row's batch; f(c, o) stores columns
// [c, c + 4) in the kernel's format
template <class F>
__device__ __forceinline__ void ln_emit(const float* __restrict__ xr, const float* __restrict__ sc, const float* __restrict__ sh, int D, int lane,
                                        float mean, float rstd, F f) {
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
    const f32x4 a = *(const f32x4*)(sc + c);
    const f32x4 bsh = *(const f32x4*)(sh + c);
    float o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (v[k] - mean) * rstd * (1.0f + a[k]) + bsh[k];
    f(c, o);
  }
}
// the modulation rows of row `rin` of segment sg: batch b = rin / rows_per_batch
__device__ __forceinline__ void ln_mod_rows(const LnSegs& segs, int sg, int rin, int mod_ld, const float*& sc, const float*& sh) {
  const int b = rin / segs.rows_per_batch[sg];
  sh = segs.shift[sg] + (size_t)b * mod_ld;
  sc = segs.scale[sg] + (size_t)b * mod_ld;
}

}  // namespace
