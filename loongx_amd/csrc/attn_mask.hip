// attn_mask.hip -- joint attention under a caller's per-(query, key) mask: the attention_mask argument of the reference's
// attn_forward (src/flux/block.py:12,101-131), which hands it to F.scaled_dot_product_attention.
//
// Operands and layout are those of lx_attn_fwd (bf16 Q / K rows, the 16-key-interleaved V^T image, up to 3 segments, the (query segment,
// key segment) bias table). The mask is in the LOGICAL order of the concatenated sequence [seg 0 | seg 1 | seg 2], shape [Bm, Hm, Sq, Sk]
// with element strides (broadcast dims of size 1). Two passes:
//
//   prep (lx_attn_mask_prep): reads the mask once, classifies every tile (mask plane, 256-row segment-local query tile, 64-key tile of the
//     padded V^T layout) as EMPTY (every valid pair masked), FULL (every valid pair attended with zero added bias) or PARTIAL, writes per query
//     tile the list of its non-EMPTY key tiles, and the per-row data of every tile: a bit per (row, key) for bool masks, an fp32 bias in
//     log2 units for float masks. Both are stored in the order the attention kernel holds its scores: position p = lhi*32 + kb*16 + r of a
//     row is key kb*32 + 8*(r>>2) + 4*lhi + (r&3) of the tile (lane half lhi, score block kb, accumulator register r), so a lane reads one
//     32-bit word of bits or 32 contiguous floats.
//   attention (lx_attn_fwd_masked): one workgroup = 8 waves = 256 query rows of one (batch, head), the work decode of lx_attn_fwd over the
//     query tiles of the segments that have queries (n_qseg / qseg_mask: the others serve keys and values only); it walks
//     the query tile's list only, so EMPTY tiles are never staged or multiplied. K [64 keys][128] and V^T [128][64 keys] tiles are staged by
//     LDS-DMA into a double buffer (one barrier per tile); S^T = K.Q^T and O^T += V^T.P^T on v_mfma_f32_32x32x16_bf16; online softmax in
//     fp32 with a running maximum (an arbitrary mask voids the bounded-score argument). FULL tiles do no mask work, PARTIAL tiles read the
//     row's bits / biases. Masked scores are a large finite negative number; a row that attends to no key is written as exact zeros (what
//     SDPA returns for it).
#include "attn_common.h"

namespace {

constexpr int MQBLK = 256;                 // query rows per tile (8 waves x 32)
constexpr float MASKED = -3.0e30f;         // score (log2 units) of a masked pair; below every attended score, which is clamped to >= -1e30
constexpr float ATT_MIN = -1.0e30f;
enum { CLS_EMPTY = 0, CLS_FULL = 1, CLS_PARTIAL = 2 };

struct MaskGeom {              // what the two passes key the workspace by; qt_start / kt_start are the AttnPlan's (lx_mask_geom)
  int n_seg;
  int seg_len[3];
  int qt_start[4];            // prefix of 256-row query tiles per segment
  int kt_start[4];            // prefix of 64-key tiles per segment (the padded V^T layout, compacted over the segments)
  int lstart[3];              // logical start of each segment in the concatenated sequence
  int n_qt, n_kt, Bm, Hm, P;  // P = Bm * Hm mask planes
  size_t list_off, cls_off, data_off, bytes;
};

struct PrepArgs {
  MaskGeom g;
  const char* mask;
  int dtype, Sq;
  long long st[4];            // element strides (0 on broadcast dims)
  float bias[3][3];           // segment-pair table: a -inf pair makes its tiles EMPTY
  int* list;
  uint8_t* cls;
  void* data;
};

// one workgroup per tile: 4 waves x 64 rows each, lane = position p of the row (key lx_vt8_key(p))
template <bool FLOAT>
__global__ __launch_bounds__(256) void lx_attn_mask_prep_kernel(const PrepArgs a) {
  const MaskGeom& g = a.g;
  const int kt = blockIdx.x, qt = blockIdx.y, plane = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sq = lx_seg_of(qt, g.qt_start, g.n_seg), sk = lx_seg_of(kt, g.kt_start, g.n_seg);
  const int q0 = (qt - g.qt_start[sq]) * MQBLK, k_in = (kt - g.kt_start[sk]) * KVBLK + lx_vt8_key(lane);
  const int lq = g.seg_len[sq], lk = g.seg_len[sk];
  const bool pair_on = a.bias[sq][sk] > -1e37f;
  const bool key_ok = pair_on && k_in < lk;
  const int bm = plane / g.Hm, hm = plane - bm * g.Hm;
  const long long kj = g.lstart[sk] + min(k_in, lk - 1);
  const char* mrow = a.mask + (bm * a.st[0] + hm * a.st[1] + kj * a.st[3]) * (a.dtype == LX_ATTN_MASK_BOOL ? 1 : a.dtype == LX_ATTN_MASK_F32 ? 4 : 2);
  const size_t tile = ((size_t)plane * g.n_qt + qt) * g.n_kt + kt;
  int att = 0, nonfull = 0;
  for (int i = wave; i < MQBLK; i += 4) {
    const bool ok = key_ok && q0 + i < lq;
    const long long qi = a.Sq == 1 ? 0 : g.lstart[sq] + min(q0 + i, lq - 1);
    bool on = false;
    float v = 0.f;
    if (ok) {
      const long long off = qi * a.st[2];
      switch (a.dtype) {
        case LX_ATTN_MASK_BOOL: on = mrow[off] != 0; break;
        case LX_ATTN_MASK_F32: v = ((const float*)mrow)[off]; break;
        case LX_ATTN_MASK_BF16: v = bf16_to_f32(((const uint16_t*)mrow)[off]); break;
        default: v = (float)((const _Float16*)mrow)[off]; break;
      }
      if (a.dtype != LX_ATTN_MASK_BOOL) on = v > -__builtin_inff();
      att |= on;
      nonfull |= !on || v != 0.f;
    }
    if constexpr (FLOAT) {
      ((float*)a.data)[(tile * MQBLK + i) * KVBLK + lane] = on ? fmaxf(v * LX_LOG2E, ATT_MIN) : MASKED;
    } else {
      const uint64_t w = __builtin_amdgcn_ballot_w64(on);
      if (lane == 0) ((uint64_t*)a.data)[tile * MQBLK + i] = w;
    }
  }
  att = __syncthreads_or(att);
  nonfull = __syncthreads_or(nonfull);
  if (threadIdx.x == 0) a.cls[tile] = !att ? CLS_EMPTY : !nonfull ? CLS_FULL : CLS_PARTIAL;
}

// one thread per (plane, query tile): the list of its non-EMPTY key tiles in key order, entry = kt | class << 16, count first
__global__ __launch_bounds__(256) void lx_attn_mask_list_kernel(const PrepArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.g.P * a.g.n_qt) return;
  const uint8_t* c = a.cls + (size_t)i * a.g.n_kt;
  int* l = a.list + (size_t)i * (a.g.n_kt + 1);
  int n = 0;
  for (int kt = 0; kt < a.g.n_kt; ++kt)
    if (c[kt] != CLS_EMPTY) l[1 + n++] = kt | ((int)c[kt] << 16);
  l[0] = n;
}

struct MaskAttnArgs {
  lx_attn_desc d;
  MaskGeom g;
  int qq_start[4];            // prefix of 256-row query tiles over the segments that HAVE queries (n_qseg / qseg_mask): the launch's items
  int wide_store;
  const int* list;
  const void* data;
};

template <bool FLOAT>
__global__ __launch_bounds__(512, 1) void lx_attn_mask_kernel(const MaskAttnArgs args) {
  constexpr int NW = 8;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_BYTES];
  const lx_attn_desc& D = args.d;
  const MaskGeom& G = args.g;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lhi = lane >> 5;
  const int BH = D.B * D.H;
  // items = the query tiles of the segments with queries only; qc counts those, qt is the tile's index among ALL segments' tiles (what
  // the prep pass keyed its lists and row data by). A segment without queries has an empty range in qq_start and is never decoded.
  int qc, bh;
  lx_item_decode((int)blockIdx.x, (int)gridDim.x, BH, args.qq_start[3], qc, bh);
  const int b = bh / D.H, h = bh % D.H;
  const int sq = lx_seg_of(qc, args.qq_start, G.n_seg);
  const int qt = G.qt_start[sq] + (qc - args.qq_start[sq]);
  const int q_len = D.seg_len[sq];
  const int q_in_seg = (qt - G.qt_start[sq]) * MQBLK + wave * 32 + l31;
  const bool q_valid = q_in_seg < q_len;
  const size_t q_row = (size_t)D.seg_row0[sq] + (size_t)b * q_len + min(q_in_seg, q_len - 1);
  const int plane = (G.Bm > 1 ? b : 0) * G.Hm + (G.Hm > 1 ? h : 0);
  const size_t qtile = (size_t)plane * G.n_qt + qt;
  const int* lst = args.list + qtile * (G.n_kt + 1);
  const int n_items = min(max(lst[0], 0), G.n_kt);   // (clamped: a list the prep pass did not write cannot send a load out of range)

  bf16x8 qf[8];
  {
    const __bf16* qp = (const __bf16*)D.Q + q_row * D.ldq + D.q_col + h * DH + lhi * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(qp + ks * 16);
  }
  const float c2 = (D.flags & LX_ATTN_Q_LOG2) ? 1.0f : D.scale * LX_LOG2E;
  f32x16 oacc[4];
  lx_zero_acc(oacc);
  float m_run = MASKED, l_run = 0.f;
  bool any = false;                      // this lane's half of the row attended to some key

  const __bf16* Kbase = (const __bf16*)D.K + D.k_col + h * DH;
  const __bf16* Vbase = (const __bf16*)D.VT + (size_t)bh * DH * D.vt_ld;
  auto entry = [&](int i, int& kt, int& sk, int& ktl, int& cls) {
    const int e = lst[1 + i];
    kt = min(max(e & 0xffff, 0), G.n_kt - 1);
    cls = e >> 16;
    sk = lx_seg_of(kt, G.kt_start, G.n_seg);
    ktl = kt - G.kt_start[sk];
  };
  // K: one instruction = 4 key rows of 256 B (lane -> row lane>>4, 16-B slot lane&15, slot ^= key&15); V^T: 8 d rows of 128 B (lane -> row
  // lane>>3, slot lane&7, slot ^= (d>>1)&7). Keys past the segment's end are staged from its last row (their probabilities are 0).
  auto stage = [&](int sk, int ktl, int buf) {
    char* base = smem + buf * STAGE_BYTES;
    const int klen = D.seg_len[sk];
    const size_t krow0 = (size_t)D.seg_row0[sk] + (size_t)b * klen;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int key = (j * NW + wave) * 4 + (lane >> 4);
      const int lslot = (lane & 15) ^ (key & 15);
      const int kin = min(ktl * KVBLK + key, klen - 1);
      const __bf16* src = Kbase + (krow0 + kin) * D.ldk + lslot * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + (j * NW + wave) * 1024), 16, 0, 0);
    }
    const int vpos = D.seg_vt0[sk] + ktl * KVBLK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int drow = (j * NW + wave) * 8 + (lane >> 3);
      const int lslot = (lane & 7) ^ ((drow >> 1) & 7);
      const __bf16* src = Vbase + (size_t)drow * D.vt_ld + vpos + lslot * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(base + K_BYTES + (j * NW + wave) * 1024), 16, 0, 0);
    }
  };
  const int ksw = l31 & 15, vsw = (l31 >> 1) & 7;
  const int k_row_off = l31 * 256, v_row_off = K_BYTES + l31 * 128;
  const int q_tile_row = wave * 32 + l31;

  int kt = 0, sk = 0, ktl = 0, cls = 0;
  if (n_items > 0) {
    entry(0, kt, sk, ktl, cls);
    stage(sk, ktl, 0);
  }
  for (int i = 0, buf = 0; i < n_items; ++i, buf ^= 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int nkt = 0, nsk = 0, nktl = 0, ncls = 0;
    if (i + 1 < n_items) {
      entry(i + 1, nkt, nsk, nktl, ncls);
      stage(nsk, nktl, buf ^ 1);
    }
    // the row's mask data of a PARTIAL tile (bits: loaded ahead of the score MFMAs; biases: after them, 32 registers)
    const size_t trow = ((qtile * G.n_kt + kt) * MQBLK + q_tile_row);
    uint32_t mbits = 0;
    if (!FLOAT && cls == CLS_PARTIAL) mbits = ((const uint32_t*)args.data)[trow * 2 + lhi];
    const char* sb = smem + buf * STAGE_BYTES;
    f32x16 sacc[2];
    lx_zero_acc(sacc);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const bf16x8 kf = *(const bf16x8*)(sb + lx_k_frag_off(kb, ks, lhi, k_row_off, ksw));
        sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[kb], 0, 0, 0);
      }
    // scores -> exp2 arguments (log2 units); score (kb, r) of this lane is key kb*32 + 8*(r>>2) + 4*lhi + (r&3) of the tile
    const float bl = D.bias[sq][sk] * LX_LOG2E;
    const int nvalid = min(KVBLK, D.seg_len[sk] - ktl * KVBLK);
    if (cls == CLS_PARTIAL) {
      f32x4 mb[8];
      if constexpr (FLOAT) {
        const f32x4* fp = (const f32x4*)((const float*)args.data + trow * KVBLK + lhi * 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) mb[j] = fp[j];
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          bool on;
          float add = bl;
          if constexpr (FLOAT) {
            const float v = mb[(kb * 16 + r) >> 2][r & 3];
            on = v > 0.5f * (MASKED + ATT_MIN);
            add += v;
          } else {
            on = (mbits >> (kb * 16 + r)) & 1;
          }
          any |= on;
          sacc[kb][r] = on ? fmaf(sacc[kb][r], c2, add) : MASKED;
        }
    } else {
      any = true;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kb][r] = fmaf(sacc[kb][r], c2, bl);
      if (nvalid < KVBLK) {              // ragged last tile of the segment (PARTIAL tiles carry these keys as masked)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kb * 32 + 8 * (r >> 2) + 4 * lhi + (r & 3) >= nvalid) sacc[kb][r] = MASKED;
      }
    }
    // online softmax, fp32, exact running maximum
    const float m_new = fmaxf(m_run, lx_tile_max(sacc));
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    l_run *= alpha;
    m_run = m_new;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[j][r] *= alpha;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(sacc[kb][r] - m_new);
        sacc[kb][r] = p;
        psum += p;
      }
    l_run += psum;
    // O^T += V^T . P^T; the P fragment of step s = accumulator registers [8*(s&1), +8) of sacc[s>>1]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(sacc[s >> 1][8 * (s & 1) + 2 * j], sacc[s >> 1][8 * (s & 1) + 2 * j + 1]);
      const bf16x8 pf = __builtin_bit_cast(bf16x8, w);
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const bf16x8 vf = *(const bf16x8*)(sb + lx_v_frag_off(db, s, lhi, v_row_off, vsw));
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[db], 0, 0, 0);
      }
    }
    kt = nkt; sk = nsk; ktl = nktl; cls = ncls;
  }
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const bool any_row = (__shfl_xor((int)any, 32, 64) | (int)any) != 0;
  if (!any_row) lx_zero_acc(oacc);       // no key attended: SDPA's exact zeros (not the uniform average of V)
  const float inv = any_row && l_tot > 0.f ? 1.0f / l_tot : 0.f;
  lx_store_o(lx_o_mode(args), (int*)D.f16_ovf, q_valid, (uint16_t*)D.O + q_row * D.ldo + D.o_col + h * DH, oacc, inv, lhi);
}

}  // namespace

static size_t lx_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the three entry points' common start: the descriptor through lx_attn_plan (the attention launch with its operands, the other two
// with the segment part only), then what is the mask's own -- dims, dtype, planes and the workspace layout. The tile prefixes are the plan's.
static int lx_mask_geom(const lx_attn_desc* d, const lx_attn_mask_desc* m, const char* who, int operands, AttnPlan& p, MaskGeom& g) {
  LX_CHECK_ARG(d && m, "%s: NULL descriptor", who);
  const int rc = lx_attn_plan(who, d, operands, 0, p);
  if (rc != LX_OK) return rc;
  LX_CHECK_ARG(m->dtype >= LX_ATTN_MASK_BOOL && m->dtype <= LX_ATTN_MASK_F16, "%s: mask dtype=%d must be LX_ATTN_MASK_BOOL / F32 / BF16 / F16", who, m->dtype);
  g.n_seg = d->n_seg;
  int S = 0;
  for (int s = 0; s < 3; ++s) {
    g.lstart[s] = S;
    g.seg_len[s] = s < d->n_seg ? d->seg_len[s] : 0;
    S += g.seg_len[s];
  }
  for (int s = 0; s < 4; ++s) {
    g.qt_start[s] = p.qt_start[s];
    g.kt_start[s] = p.kt_start[s];
  }
  g.n_qt = p.qt_start[3];
  g.n_kt = p.kt_start[3];
  LX_CHECK_ARG(g.n_kt < 65536, "%s: %d key tiles (at most 65535)", who, g.n_kt);
  const int* dm = m->dims;
  LX_CHECK_ARG((dm[0] == 1 || dm[0] == d->B) && (dm[1] == 1 || dm[1] == d->H) && (dm[2] == 1 || dm[2] == S) && dm[3] == S,
               "%s: mask dims [%d, %d, %d, %d] must be [1|B, 1|H, 1|S, S] with B=%d H=%d S=%d", who, dm[0], dm[1], dm[2], dm[3], d->B, d->H, S);
  for (int i = 0; i < 4; ++i) LX_CHECK_ARG(m->strides[i] >= 0, "%s: mask stride %d is negative", who, i);
  g.Bm = dm[0];
  g.Hm = dm[1];
  g.P = g.Bm * g.Hm;
  const size_t tiles = (size_t)g.P * g.n_qt * g.n_kt;
  g.list_off = 0;
  g.cls_off = lx_align256((size_t)g.P * g.n_qt * (g.n_kt + 1) * sizeof(int));
  g.data_off = g.cls_off + lx_align256(tiles);
  g.bytes = g.data_off + tiles * MQBLK * (m->dtype == LX_ATTN_MASK_BOOL ? sizeof(uint64_t) : KVBLK * sizeof(float));
  return LX_OK;
}

static int lx_mask_ws_check(const lx_attn_mask_desc* m, const MaskGeom& g, const char* who) {
  LX_CHECK_ARG(m->workspace && ((uintptr_t)m->workspace & 255) == 0, "%s: workspace must be non-NULL and 256-byte aligned", who);
  LX_CHECK_ARG(m->workspace_bytes >= g.bytes, "%s: workspace of %zu bytes, %zu needed (lx_attn_mask_workspace)", who, m->workspace_bytes, g.bytes);
  return LX_OK;
}

extern "C" int lx_attn_mask_workspace(const lx_attn_desc* d, const lx_attn_mask_desc* m, size_t* bytes) {
  AttnPlan p;
  MaskGeom g;
  const int st = lx_mask_geom(d, m, "lx_attn_mask_workspace", LX_ATTN_SEGMENTS_ONLY, p, g);
  if (st != LX_OK) return st;
  LX_CHECK_ARG(bytes, "lx_attn_mask_workspace: NULL result pointer");
  *bytes = g.bytes;
  return LX_OK;
}

extern "C" int lx_attn_mask_prep(const lx_attn_desc* d, const lx_attn_mask_desc* m, void* stream) {
  AttnPlan p;
  MaskGeom g;
  int st = lx_mask_geom(d, m, "lx_attn_mask_prep", LX_ATTN_SEGMENTS_ONLY, p, g);
  if (st != LX_OK) return st;
  LX_CHECK_ARG(m->mask, "lx_attn_mask_prep: NULL mask");
  if ((st = lx_mask_ws_check(m, g, "lx_attn_mask_prep")) != LX_OK) return st;
  PrepArgs a;
  a.g = g;
  a.mask = (const char*)m->mask;
  a.dtype = m->dtype;
  a.Sq = m->dims[2];
  for (int i = 0; i < 4; ++i) a.st[i] = m->dims[i] == 1 ? 0 : m->strides[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a.bias[i][j] = d->bias[i][j];
  char* ws = (char*)m->workspace;
  a.list = (int*)(ws + g.list_off);
  a.cls = (uint8_t*)(ws + g.cls_off);
  a.data = ws + g.data_off;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g.n_kt, g.n_qt, g.P);
  if (m->dtype == LX_ATTN_MASK_BOOL) hipLaunchKernelGGL(lx_attn_mask_prep_kernel<false>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(lx_attn_mask_prep_kernel<true>, grid, dim3(256), 0, s, a);
  LX_LAUNCH_CHECK("lx_attn_mask_prep");
  hipLaunchKernelGGL(lx_attn_mask_list_kernel, dim3((g.P * g.n_qt + 255) / 256), dim3(256), 0, s, a);
  LX_LAUNCH_CHECK("lx_attn_mask_prep (list)");
  return LX_OK;
}

extern "C" int lx_attn_fwd_masked(const lx_attn_desc* d, const lx_attn_mask_desc* m, void* stream) {
  AttnPlan p;
  MaskGeom g;
  int st = lx_mask_geom(d, m, "lx_attn_fwd_masked", LX_ATTN_OPERANDS_16BIT, p, g);
  if (st != LX_OK) return st;
  LX_CHECK_ARG((d->flags & ~(LX_ATTN_Q_LOG2 | LX_ATTN_O_F16)) == 0, "lx_attn_fwd_masked: flags=%d: only LX_ATTN_Q_LOG2 and LX_ATTN_O_F16 are accepted", d->flags);
  if ((st = lx_mask_ws_check(m, g, "lx_attn_fwd_masked")) != LX_OK) return st;
  MaskAttnArgs a;
  a.d = *d;
  a.g = g;
  a.wide_store = p.wide_store;
  a.list = (const int*)((const char*)m->workspace + g.list_off);
  a.data = (const char*)m->workspace + g.data_off;
  // The prep pass classified every query tile; this launch covers the tiles of the query segments only.
  for (int i = 0; i < 4; ++i) a.qq_start[i] = p.qq_start[i];
  const int grid = p.items;
  hipStream_t s = (hipStream_t)stream;
  if (m->dtype == LX_ATTN_MASK_BOOL) hipLaunchKernelGGL(lx_attn_mask_kernel<false>, dim3(grid), dim3(512), 0, s, a);
  else hipLaunchKernelGGL(lx_attn_mask_kernel<true>, dim3(grid), dim3(512), 0, s, a);
  LX_LAUNCH_CHECK("lx_attn_fwd_masked");
  return LX_OK;
}
