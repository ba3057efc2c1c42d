// step.hip -- the scheduler step (gfx950): the Euler step on one, two or three branches of the velocity, the inpaint blend, the img2img
// start (lx_scale_noise), adaptive projected guidance, the second-order multistep term (DPM-Solver++(2M)) and FlowEdit's two launches
// (lx_flowedit_inputs, lx_flowedit_step), which share the item loop and the load / store parts. One operation written once:
// a further guidance variant is a PARTS value or a term in guided_v, and a thin entry point. The operation order is the contract of
// include/lx.h: every rounding below is spelled out (__fsub_rn / __fmul_rn / fmaf), so that no contraction setting can move one.
#include "common.h"

namespace {

// W consecutive elements of one part: W = 4 moves 16 bytes at a time (8 of a bf16 v), W = 1 one element
template <int W>
struct Item { float e[W]; };

template <int W>
__device__ __forceinline__ Item<W> load_f32(const float* __restrict__ p, size_t i) {
  if constexpr (W == 4) {
    const f32x4 t = *(const f32x4*)(p + i);
    return Item<4>{{t[0], t[1], t[2], t[3]}};
  } else {
    return Item<1>{{p[i]}};
  }
}
// v is fp32 or bf16
template <int W>
__device__ __forceinline__ Item<W> load_v(const void* __restrict__ v, int v_bf16, size_t i) {
  if (!v_bf16) return load_f32<W>((const float*)v, i);
  if constexpr (W == 4) {
    const u32x2 p = *(const u32x2*)((const uint16_t*)v + i);
    return Item<4>{{bf16_to_f32((uint16_t)(p[0] & 0xffffu)), bf16_to_f32((uint16_t)(p[0] >> 16)),
                    bf16_to_f32((uint16_t)(p[1] & 0xffffu)), bf16_to_f32((uint16_t)(p[1] >> 16))}};
  } else {
    return Item<1>{{bf16_to_f32(((const uint16_t*)v)[i])}};
  }
}
template <int W>
__device__ __forceinline__ void store_f32(float* __restrict__ p, size_t i, const Item<W>& o) {
  if constexpr (W == 4) *(f32x4*)(p + i) = f32x4{o.e[0], o.e[1], o.e[2], o.e[3]};
  else p[i] = o.e[0];
}
// the result of a step goes to every part of x
template <int W>
__device__ __forceinline__ void store_parts(float* __restrict__ x, int parts, size_t n, size_t i, const Item<W>& o) {
  for (int p = 0; p < parts; ++p) store_f32<W>(x, (size_t)p * n + i, o);
}

// The velocity the step runs along. One part: v0. Two, [positive; negative] or [full; text]: v1 + scale_a (v0 - v1). Three,
// [full; text; negative]: v2 + scale_b (g - v2) with g the two-part value of (v0, v1). The difference is rounded on its own; v0 == v1 bit for
// bit makes g == v1 exactly (0 * scale_a + v1; the scale is finite), so three parts with vF == vT are two parts on (vT, vN).
template <int PARTS>
__device__ __forceinline__ float guided_v(float v0, float v1, float v2, float scale_a, float scale_b) {
  if constexpr (PARTS == 1) {
    return v0;
  } else {
    const float g = fmaf(scale_a, __fsub_rn(v0, v1), v1);
    if constexpr (PARTS == 2) return g;
    else return fmaf(scale_b, __fsub_rn(g, v2), v2);
  }
}
// guided_v of the W elements at i of PARTS parts of n elements; v0 receives the first part's
template <int W, int PARTS>
__device__ __forceinline__ Item<W> guided_item(const void* __restrict__ v, int v_bf16, size_t n, size_t i, float scale_a, float scale_b,
                                               Item<W>& v0) {
  v0 = load_v<W>(v, v_bf16, i);
  const Item<W> v1 = PARTS > 1 ? load_v<W>(v, v_bf16, n + i) : v0;
  const Item<W> v2 = PARTS > 2 ? load_v<W>(v, v_bf16, 2 * n + i) : v1;
  Item<W> g;
#pragma unroll
  for (int j = 0; j < W; ++j) g.e[j] = guided_v<PARTS>(v0.e[j], v1.e[j], v2.e[j], scale_a, scale_b);
  return g;
}

__device__ __forceinline__ float scale_noise1(float x0, float z, float sigma, float one_minus_sigma) {
  return fmaf(sigma, z, __fmul_rn(one_minus_sigma, x0));
}
// the stepped value e blended with the source noised to the next level
__device__ __forceinline__ float blend1(float e, float x0, float z, float m, float sigma_next, float one_minus_sigma) {
  const float r = scale_noise1(x0, z, sigma_next, one_minus_sigma);
  return fmaf(m, e, __fmul_rn(__fsub_rn(1.f, m), r));
}
// the inpaint operands of a step: one part's element count each (all NULL where the kernel is not a BLEND one)
struct Blend {
  const float* x0; const float* z; const float* m;
  float sigma_next, one_minus_sigma;
};
template <int W>
__device__ __forceinline__ void blend_item(Item<W>& o, const Blend& bl, size_t i) {
  const Item<W> a = load_f32<W>(bl.x0, i), b = load_f32<W>(bl.z, i), mm = load_f32<W>(bl.m, i);
#pragma unroll
  for (int j = 0; j < W; ++j) o.e[j] = blend1(o.e[j], a.e[j], b.e[j], mm.e[j], bl.sigma_next, bl.one_minus_sigma);
}

// the second-order operands of a step (lx_dpmpp2m_step, lx_dpmpp2m_step_apg): the previous step's denoised prediction D (fp32, one part's
// element count, updated in place) and the coefficient c of its difference. All unused where the kernel is not a MULTI one.
struct Multi {
  float* D;
  float c, neg_sigma;
};
// o, the Euler value of x along g, receives c (d - D[i]) with d = x - sigma g the denoised prediction, which replaces D[i]. A work item reads
// and then writes only its own elements of D. c == 0 (uniform over the launch) does not read D: the Euler value leaves as it came, and
// whatever D held, a NaN included, is overwritten.
template <int W>
__device__ __forceinline__ void multi_item(Item<W>& o, const Item<W>& x, const Item<W>& g, const Multi& ms, size_t i) {
  Item<W> d;
#pragma unroll
  for (int j = 0; j < W; ++j) d.e[j] = fmaf(ms.neg_sigma, g.e[j], x.e[j]);
  if (ms.c != 0.f) {
    const Item<W> prev = load_f32<W>(ms.D, i);
#pragma unroll
    for (int j = 0; j < W; ++j) o.e[j] = fmaf(ms.c, __fsub_rn(d.e[j], prev.e[j]), o.e[j]);
  }
  store_f32<W>(ms.D, i, d);
}

// ---- the step (lx_euler_step, lx_euler_step_blend, lx_euler_step_cfg, lx_euler_step_cfg3, lx_dpmpp2m_step) ---------------------------------
// x and v hold PARTS parts of n elements. e = x[0, n) + ds guided_v, the second-order term where MULTI, the inpaint blend where BLEND, and
// the result stored to every part of x. A work item is VEC consecutive elements of one part, grid-stride loop under a capped grid. VEC = 4:
// the last n % 4 elements go one by one; with PARTS > 1 the host takes it only where n % 4 == 0 (the later parts are aligned only there),
// so that tail is dead.
template <int W, int PARTS, bool BLEND, bool MULTI>
__device__ __forceinline__ void step_item(float* __restrict__ x, const void* __restrict__ v, int v_bf16, float ds, float scale_a, float scale_b,
                                          const Blend& bl, const Multi& ms, size_t n, size_t i) {
  Item<W> v0;
  const Item<W> g = guided_item<W, PARTS>(v, v_bf16, n, i, scale_a, scale_b, v0), xx = load_f32<W>(x, i);
  Item<W> o;
#pragma unroll
  for (int j = 0; j < W; ++j) o.e[j] = fmaf(ds, g.e[j], xx.e[j]);
  if constexpr (MULTI) multi_item<W>(o, xx, g, ms, i);
  if constexpr (BLEND) blend_item<W>(o, bl, i);
  store_parts<W>(x, PARTS, n, i, o);
}

template <int VEC, int PARTS, bool BLEND, bool MULTI>
__global__ __launch_bounds__(256) void euler_parts_kernel(float* __restrict__ x, const void* __restrict__ v, int v_bf16, float ds, float scale_a,
                                                          float scale_b, const Blend bl, size_t n, const Multi ms) {
  const size_t items = (n + VEC - 1) / VEC, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t i = it * VEC;
    if (VEC == 4 && i + 4 <= n) {
      step_item<4, PARTS, BLEND, MULTI>(x, v, v_bf16, ds, scale_a, scale_b, bl, ms, n, i);
    } else {
      for (size_t k = i; k < n && k < i + VEC; ++k) step_item<1, PARTS, BLEND, MULTI>(x, v, v_bf16, ds, scale_a, scale_b, bl, ms, n, k);
    }
  }
}

// ---- the img2img start (lx_scale_noise): no v, and it writes out, not x; the step's item loop -----------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void scale_noise_kernel(float* __restrict__ out, const float* __restrict__ x0, const float* __restrict__ z,
                                                          float sigma, float one_minus_sigma, size_t n) {
  const size_t items = (n + VEC - 1) / VEC, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t i = it * VEC;
    if (VEC == 4 && i + 4 <= n) {
      const Item<4> a = load_f32<4>(x0, i), b = load_f32<4>(z, i);
      Item<4> o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.e[j] = scale_noise1(a.e[j], b.e[j], sigma, one_minus_sigma);
      store_f32<4>(out, i, o);
    } else {
      for (size_t k = i; k < n && k < i + VEC; ++k) out[k] = scale_noise1(x0[k], z[k], sigma, one_minus_sigma);
    }
  }
}

// ---- FlowEdit (lx_flowedit_inputs, lx_flowedit_step): the step's item loop on two-part arrays ------------------------------------------
// The inputs of one forward: s = the source noised to sigma (scale_noise1: lx_scale_noise's bits) to out[n + i], z_fe + (s - x_src) to
// out[i]. The host takes VEC = 4 only where n % 4 == 0 (the second part is aligned only there), so the element tail is dead on that path.
template <int W>
__device__ __forceinline__ void flowedit_inputs_item(float* __restrict__ out, const float* __restrict__ x_src, const float* __restrict__ z_fe,
                                                     const float* __restrict__ noise, float sigma, float one_minus_sigma, size_t n, size_t i) {
  const Item<W> a = load_f32<W>(x_src, i), b = load_f32<W>(noise, i), zz = load_f32<W>(z_fe, i);
  Item<W> s, r;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    s.e[j] = scale_noise1(a.e[j], b.e[j], sigma, one_minus_sigma);
    r.e[j] = __fadd_rn(zz.e[j], __fsub_rn(s.e[j], a.e[j]));
  }
  store_f32<W>(out, i, r);
  store_f32<W>(out, n + i, s);
}

template <int VEC>
__global__ __launch_bounds__(256) void flowedit_inputs_kernel(float* __restrict__ out, const float* __restrict__ x_src,
                                                              const float* __restrict__ z_fe, const float* __restrict__ noise, float sigma,
                                                              float one_minus_sigma, size_t n) {
  const size_t items = (n + VEC - 1) / VEC, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t i = it * VEC;
    if (VEC == 4 && i + 4 <= n) {
      flowedit_inputs_item<4>(out, x_src, z_fe, noise, sigma, one_minus_sigma, n, i);
    } else {
      for (size_t k = i; k < n && k < i + VEC; ++k) flowedit_inputs_item<1>(out, x_src, z_fe, noise, sigma, one_minus_sigma, n, k);
    }
  }
}

// The update after one forward on [target; source]: z_fe += coef (m) (vt - vs). An element with m == 0 is stored as it was read.
template <int W, bool MASK>
__device__ __forceinline__ void flowedit_step_item(float* __restrict__ z_fe, const void* __restrict__ v, int v_bf16, float coef,
                                                   const float* __restrict__ m, size_t n, size_t i) {
  const Item<W> vt = load_v<W>(v, v_bf16, i), vs = load_v<W>(v, v_bf16, n + i), zz = load_f32<W>(z_fe, i);
  Item<W> mm = zz, o;
  if constexpr (MASK) mm = load_f32<W>(m, i);
#pragma unroll
  for (int j = 0; j < W; ++j) {
    float d = __fsub_rn(vt.e[j], vs.e[j]);
    if constexpr (MASK) d = __fmul_rn(mm.e[j], d);
    const float r = fmaf(coef, d, zz.e[j]);
    o.e[j] = (MASK && mm.e[j] == 0.f) ? zz.e[j] : r;
  }
  store_f32<W>(z_fe, i, o);
}

template <int VEC, bool MASK>
__global__ __launch_bounds__(256) void flowedit_step_kernel(float* __restrict__ z_fe, const void* __restrict__ v, int v_bf16, float coef,
                                                            const float* __restrict__ m, size_t n) {
  const size_t items = (n + VEC - 1) / VEC, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += stride) {
    const size_t i = it * VEC;
    if (VEC == 4 && i + 4 <= n) {
      flowedit_step_item<4, MASK>(z_fe, v, v_bf16, coef, m, n, i);
    } else {
      for (size_t k = i; k < n && k < i + VEC; ++k) flowedit_step_item<1, MASK>(z_fe, v, v_bf16, coef, m, n, k);
    }
  }
}

// ---- the guided step under adaptive projected guidance (lx_euler_step_apg) -----------------------------------------------------------
// Three launches, the order of include/lx.h. An image is cut into chunks of APG_CHUNK elements; block (chunk, image) owns one chunk, so no
// chunk straddles two images. Within a chunk thread t owns the 4 elements at 1024 r + 4 t, r = 0..3, on the 16-byte path and on the element
// path alike, and adds their products in (r, element) order: the two paths give the same bits.
//   apg_reduce_kernel  Db of every element to M, and the chunk's (sum Db^2, sum Db w, sum w^2) in double to the workspace: per thread in its
//                      fixed order, across the lanes of a wave by the xor tree, across the four waves in wave order by thread 0.
//   apg_total_kernel   per image, the chunk triples added in chunk order. No atomics anywhere: the same bits from run to run.
//   apg_step_kernel    reads the image's sums, forms the two fp32 coefficients, projects, steps (with the second-order term around the
//                      projected velocity where MULTI: lx_dpmpp2m_step_apg), blends and stores to every part.
constexpr int APG_CHUNK = 4096;

// Db = -sigma (guided_v - v0) (+ momentum M) of the W elements at i, stored to M; xi, vc and db receive x, v0 and Db for the sums
template <int W, int PARTS>
__device__ __forceinline__ void apg_reduce_item(const float* __restrict__ x, const void* __restrict__ v, int v_bf16, float scale_a, float scale_b,
                                                float neg_sigma, float momentum, float* __restrict__ M, size_t n, size_t i, float* xi, float* vc,
                                                float* db) {
  Item<W> v0;
  const Item<W> g = guided_item<W, PARTS>(v, v_bf16, n, i, scale_a, scale_b, v0), xx = load_f32<W>(x, i);
  Item<W> d;
#pragma unroll
  for (int j = 0; j < W; ++j) d.e[j] = __fmul_rn(neg_sigma, __fsub_rn(g.e[j], v0.e[j]));
  if (momentum != 0.f) {
    const Item<W> mm = load_f32<W>(M, i);
#pragma unroll
    for (int j = 0; j < W; ++j) d.e[j] = fmaf(momentum, mm.e[j], d.e[j]);
  }
  store_f32<W>(M, i, d);
#pragma unroll
  for (int j = 0; j < W; ++j) {
    xi[j] = xx.e[j];
    vc[j] = v0.e[j];
    db[j] = d.e[j];
  }
}

template <int VEC, int PARTS>
__global__ __launch_bounds__(256) void apg_reduce_kernel(const float* __restrict__ x, const void* __restrict__ v, int v_bf16, float scale_a,
                                                         float scale_b, float neg_sigma, float momentum, float* __restrict__ M,
                                                         double* __restrict__ partials, size_t elems, size_t n) {
  const size_t base = (size_t)blockIdx.y * elems, c0 = (size_t)blockIdx.x * APG_CHUNK;
  double sdd = 0.0, sdw = 0.0, sww = 0.0;
  for (int r = 0; r < 4; ++r) {
    const size_t e = c0 + (size_t)r * 1024 + (size_t)threadIdx.x * 4;
    if (e >= elems) break;
    const size_t i = base + e;
    const int cnt = elems - e < 4 ? (int)(elems - e) : 4;               // (4 on the 16-byte path: elems % 4 == 0 there)
    float xi[4], vc[4], db[4];
    if (VEC == 4) {
      apg_reduce_item<4, PARTS>(x, v, v_bf16, scale_a, scale_b, neg_sigma, momentum, M, n, i, xi, vc, db);
    } else {
      for (int j = 0; j < cnt; ++j)
        apg_reduce_item<1, PARTS>(x, v, v_bf16, scale_a, scale_b, neg_sigma, momentum, M, n, i + j, xi + j, vc + j, db + j);
    }
    for (int j = 0; j < cnt; ++j) {
      const double d = (double)db[j], w = (double)fmaf(neg_sigma, vc[j], xi[j]);      // (products of two fp32 values: exact in double)
      sdd += d * d;
      sdw += d * w;
      sww += w * w;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sdd += __shfl_xor(sdd, o, 64);
    sdw += __shfl_xor(sdw, o, 64);
    sww += __shfl_xor(sww, o, 64);
  }
  __shared__ double wave_sums[4][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    wave_sums[wave][0] = sdd;
    wave_sums[wave][1] = sdw;
    wave_sums[wave][2] = sww;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double* out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    out[threadIdx.x] = ((wave_sums[0][threadIdx.x] + wave_sums[1][threadIdx.x]) + wave_sums[2][threadIdx.x]) + wave_sums[3][threadIdx.x];
  }
}

// one wave per image; lane k < 3 adds component k of the image's chunk triples in chunk order
__global__ __launch_bounds__(64) void apg_total_kernel(const double* __restrict__ partials, int chunks, double* __restrict__ sums) {
  if (threadIdx.x >= 3) return;
  const double* p = partials + (size_t)blockIdx.x * chunks * 3 + threadIdx.x;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[(size_t)c * 3];
  sums[(size_t)blockIdx.x * 3 + threadIdx.x] = s;
}

// the fp32 values of a projected step that are the same for every element of an image
struct ApgCoef { float neg_sigma, c32, k32, neg_inv_sigma, ds; };

// the projected velocity the step runs along
__device__ __forceinline__ float apg_velocity1(float x, float vc, float db, const ApgCoef& a) {
  const float w = fmaf(a.neg_sigma, vc, x);
  const float u = fmaf(a.c32, db, -__fmul_rn(a.k32, w));
  return fmaf(a.neg_inv_sigma, u, vc);
}
template <int W, bool BLEND, bool MULTI>
__device__ __forceinline__ void apg_step_item(float* __restrict__ x, const void* __restrict__ v, int v_bf16, int parts, const ApgCoef& a,
                                              const float* __restrict__ M, const Blend& bl, const Multi& ms, size_t n, size_t i) {
  const Item<W> vc = load_v<W>(v, v_bf16, i), db = load_f32<W>(M, i), xx = load_f32<W>(x, i);
  Item<W> g, o;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    g.e[j] = apg_velocity1(xx.e[j], vc.e[j], db.e[j], a);
    o.e[j] = fmaf(a.ds, g.e[j], xx.e[j]);
  }
  if constexpr (MULTI) multi_item<W>(o, xx, g, ms, i);
  if constexpr (BLEND) blend_item<W>(o, bl, i);
  store_parts<W>(x, parts, n, i, o);
}

template <int VEC, bool BLEND, bool MULTI>
__global__ __launch_bounds__(256) void apg_step_kernel(float* __restrict__ x, const void* __restrict__ v, int v_bf16, int parts,
                                                       float neg_sigma, float neg_inv_sigma, float ds, float eta, float norm_threshold,
                                                       const float* __restrict__ M, const double* __restrict__ sums, const Blend bl,
                                                       size_t elems, size_t n, const Multi ms) {
  const double sdd = sums[(size_t)blockIdx.y * 3], sdw = sums[(size_t)blockIdx.y * 3 + 1], sww = sums[(size_t)blockIdx.y * 3 + 2];
  const double r = (double)norm_threshold;
  const double c = (norm_threshold > 0.f && sdd > r * r) ? r / sqrt(sdd) : 1.0;
  const double a = sww > 0.0 ? sdw / sww : 0.0;
  const ApgCoef coef{neg_sigma, (float)c, (float)((c * (1.0 - (double)eta)) * a), neg_inv_sigma, ds};
  const size_t base = (size_t)blockIdx.y * elems, c0 = (size_t)blockIdx.x * APG_CHUNK;
  for (int rr = 0; rr < 4; ++rr) {
    const size_t e = c0 + (size_t)rr * 1024 + (size_t)threadIdx.x * 4;
    if (e >= elems) break;
    const size_t i = base + e;
    if (VEC == 4) {
      apg_step_item<4, BLEND, MULTI>(x, v, v_bf16, parts, coef, M, bl, ms, n, i);
    } else {
      const int cnt = elems - e < 4 ? (int)(elems - e) : 4;
      for (int j = 0; j < cnt; ++j) apg_step_item<1, BLEND, MULTI>(x, v, v_bf16, parts, coef, M, bl, ms, n, i + j);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool f32_is_finite(float f) {
  uint32_t bits;
  __builtin_memcpy(&bits, &f, sizeof bits);
  return (bits & 0x7f800000u) != 0x7f800000u;
}

// The aliasing rules of an in-place step on x[0, xbytes), in the entries' order: x0, z and m (pbytes each; checked where m is given), then
// v where check_v (an fp32 v of x's size; a bf16 v cannot be x). `xrange` is how the entry's texts name x's extent.
int check_step_aliases(const char* name, const char* xrange, const float* x, size_t xbytes, const void* v, bool check_v, const float* x0,
                       const float* z, const float* m, size_t pbytes) {
  LX_CHECK_ARG(!m || (!byte_ranges_overlap(x, xbytes, x0, pbytes) && !byte_ranges_overlap(x, xbytes, z, pbytes) &&
                      !byte_ranges_overlap(x, xbytes, m, pbytes)),
               "%s: x0, z and m may not alias %s (it is updated in place)", name, xrange);
  LX_CHECK_ARG(!check_v || !byte_ranges_overlap(x, xbytes, v, xbytes), "%s: v may not alias %s", name, xrange);
  return LX_OK;
}

// The aliasing rules of the second-order history D (pbytes: one part, read and written in place): not x, not v (fp32 or bf16: v is read
// by other work items while D is written), not the blend's operands.
int check_multi_aliases(const char* name, const char* xrange, const float* D, const float* x, size_t xbytes, const void* v, size_t vbytes,
                        const float* x0, const float* z, const float* m, size_t pbytes) {
  LX_CHECK_ARG(!byte_ranges_overlap(D, pbytes, x, xbytes), "%s: D may not overlap %s", name, xrange);
  LX_CHECK_ARG(!byte_ranges_overlap(D, pbytes, v, vbytes), "%s: D may not overlap v (it is written while v is read)", name);
  LX_CHECK_ARG(!m || (!byte_ranges_overlap(D, pbytes, x0, pbytes) && !byte_ranges_overlap(D, pbytes, z, pbytes) &&
                      !byte_ranges_overlap(D, pbytes, m, pbytes)),
               "%s: D may not overlap x0, z or m", name);
  return LX_OK;
}

// x0, z and m are given together or not at all
bool blend_triple_ok(const float* x0, const float* z, const float* m) { return (x0 && z && m) || (!x0 && !z && !m); }

// The 16-byte path: every part of every operand starts aligned. part_stride is the distance between two part (or image) starts of x and
// v, 0 where there is one; f32_ptrs the fp32 operands' addresses or'ed together (NULL ones add nothing); v needs 8 bytes as bf16.
bool step_vec16(size_t part_stride, uintptr_t f32_ptrs, const void* v, int v_is_bf16) {
  return part_stride % 4 == 0 && (f32_ptrs & 15) == 0 && ((uintptr_t)v & (v_is_bf16 ? 7 : 15)) == 0;
}
uintptr_t addr_bits(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                    const void* f = nullptr) {
  return (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f;
}

int step_grid(size_t items) { return (int)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048); }

template <int VEC, int PARTS, bool BLEND, bool MULTI = false>
void launch_parts(float* x, const void* v, int v_is_bf16, float dsigma, float scale_a, float scale_b, const Blend& bl, size_t n,
                  hipStream_t stream, const Multi& ms = Multi{}) {
  hipLaunchKernelGGL((euler_parts_kernel<VEC, PARTS, BLEND, MULTI>), dim3(step_grid((n + VEC - 1) / VEC)), dim3(256), 0, stream, x, v,
                     v_is_bf16, dsigma, scale_a, scale_b, bl, n, ms);
}
// the guided step on PARTS parts of n elements: the blend where m is given, 16 bytes at a time where vec, the second-order term where MULTI
template <int PARTS, bool MULTI = false>
void launch_step(float* x, const void* v, int v_is_bf16, float dsigma, float scale_a, float scale_b, const float* x0, const float* z,
                 const float* m, float sigma_next, size_t n, bool vec, hipStream_t stream, const Multi& ms = Multi{}) {
  const Blend bl{x0, z, m, sigma_next, 1.0f - sigma_next};
  if (vec && m) launch_parts<4, PARTS, true, MULTI>(x, v, v_is_bf16, dsigma, scale_a, scale_b, bl, n, stream, ms);
  else if (vec) launch_parts<4, PARTS, false, MULTI>(x, v, v_is_bf16, dsigma, scale_a, scale_b, bl, n, stream, ms);
  else if (m) launch_parts<1, PARTS, true, MULTI>(x, v, v_is_bf16, dsigma, scale_a, scale_b, bl, n, stream, ms);
  else launch_parts<1, PARTS, false, MULTI>(x, v, v_is_bf16, dsigma, scale_a, scale_b, bl, n, stream, ms);
}

// chunks of one image; 0 where n_images x chunks x 3 doubles, or 3 parts of n_images x elems floats, do not fit an address
size_t apg_chunks(int n_images, size_t elems) {
  if (n_images < 1 || n_images > 65535 || elems == 0) return 0;
  if (elems > SIZE_MAX / (3 * sizeof(float)) / (size_t)n_images) return 0;
  const size_t chunks = (elems + APG_CHUNK - 1) / APG_CHUNK;
  return chunks <= 0x7fffffffu ? chunks : 0;
}

size_t apg_workspace(int n_images, size_t elems) {
  return apg_chunks(n_images, elems) * (size_t)(n_images > 0 ? n_images : 0) * 3 * sizeof(double);
}

template <int VEC>
void launch_apg(float* x, const void* v, int v_is_bf16, int n_parts, float scale_a, float scale_b, float sigma, float dsigma, float eta,
                float norm_threshold, float momentum, float* M, double* sums, double* partials, const Blend& bl, int n_images, size_t elems,
                hipStream_t stream, const Multi* ms) {
  const size_t n = (size_t)n_images * elems;
  const int chunks = (int)apg_chunks(n_images, elems);
  const dim3 grid(chunks, n_images);
  const float neg_sigma = -sigma, neg_inv_sigma = -(1.0f / sigma);
  if (n_parts == 2) hipLaunchKernelGGL((apg_reduce_kernel<VEC, 2>), grid, dim3(256), 0, stream, x, v, v_is_bf16, scale_a, scale_b, neg_sigma, momentum, M, partials, elems, n);
  else hipLaunchKernelGGL((apg_reduce_kernel<VEC, 3>), grid, dim3(256), 0, stream, x, v, v_is_bf16, scale_a, scale_b, neg_sigma, momentum, M, partials, elems, n);
  hipLaunchKernelGGL(apg_total_kernel, dim3(n_images), dim3(64), 0, stream, (const double*)partials, chunks, sums);
  const Multi none{};
  if (ms && bl.m) hipLaunchKernelGGL((apg_step_kernel<VEC, true, true>), grid, dim3(256), 0, stream, x, v, v_is_bf16, n_parts, neg_sigma, neg_inv_sigma, dsigma, eta, norm_threshold, M, sums, bl, elems, n, *ms);
  else if (ms) hipLaunchKernelGGL((apg_step_kernel<VEC, false, true>), grid, dim3(256), 0, stream, x, v, v_is_bf16, n_parts, neg_sigma, neg_inv_sigma, dsigma, eta, norm_threshold, M, sums, bl, elems, n, *ms);
  else if (bl.m) hipLaunchKernelGGL((apg_step_kernel<VEC, true, false>), grid, dim3(256), 0, stream, x, v, v_is_bf16, n_parts, neg_sigma, neg_inv_sigma, dsigma, eta, norm_threshold, M, sums, bl, elems, n, none);
  else hipLaunchKernelGGL((apg_step_kernel<VEC, false, false>), grid, dim3(256), 0, stream, x, v, v_is_bf16, n_parts, neg_sigma, neg_inv_sigma, dsigma, eta, norm_threshold, M, sums, bl, elems, n, none);
}

// lx_euler_step_apg (D == NULL: no second-order term) and lx_dpmpp2m_step_apg under their own names: the checks, the 16-byte decision and
// the three launches
int apg_entry(const char* name, float* x, const void* v, int v_is_bf16, int n_parts, float scale_a, float scale_b, float sigma, float dsigma,
              const Multi* ms, float eta, float norm_threshold, float momentum, float* M, double* sums, void* workspace, size_t workspace_bytes,
              const float* x0, const float* z, const float* m, float sigma_next, int n_images, size_t elems, void* stream) {
  if (ms) LX_CHECK_ARG(x && v && M && sums && workspace && ms->D, "%s: NULL x, v, D, M, sums or workspace", name);
  else LX_CHECK_ARG(x && v && M && sums && workspace, "%s: NULL x, v, M, sums or workspace", name);
  LX_CHECK_ARG(n_parts == 2 || n_parts == 3, "%s: n_parts=%d must be 2 or 3", name, n_parts);
  LX_CHECK_ARG(n_images >= 1 && elems > 0, "%s: n_images < 1 or elems == 0", name);
  LX_CHECK_ARG(apg_chunks(n_images, elems) > 0, "%s: more than 65535 images, or the parts do not fit an address", name);
  LX_CHECK_ARG(f32_is_finite(sigma) && sigma > 0.f, "%s: sigma must be finite and > 0", name);
  LX_CHECK_ARG(f32_is_finite(scale_a) && (n_parts == 2 || f32_is_finite(scale_b)), "%s: a scale is not finite", name);
  LX_CHECK_ARG(!ms || f32_is_finite(ms->c), "%s: c is not finite", name);
  LX_CHECK_ARG(f32_is_finite(eta) && f32_is_finite(norm_threshold) && f32_is_finite(momentum),
               "%s: eta, norm_threshold or momentum is not finite", name);
  LX_CHECK_ARG(eta >= 0.f && eta <= 1.f, "%s: eta must lie in [0, 1]", name);
  LX_CHECK_ARG(norm_threshold >= 0.f, "%s: norm_threshold must be >= 0", name);
  LX_CHECK_ARG(momentum > -1.f && momentum < 1.f, "%s: |momentum| must be < 1", name);
  LX_CHECK_ARG(blend_triple_ok(x0, z, m), "%s: x0, z and m go together (all NULL: no blend)", name);
  LX_CHECK_ARG(workspace_bytes >= apg_workspace(n_images, elems), "%s: the workspace is smaller than lx_apg_workspace_bytes", name);
  LX_CHECK_ARG((addr_bits(workspace, sums) & 7) == 0, "%s: the workspace and sums must be 8-byte aligned", name);
  const size_t n = (size_t)n_images * elems, xbytes = (size_t)n_parts * n * sizeof(float), pbytes = n * sizeof(float);
  const size_t vbytes = (size_t)n_parts * n * (v_is_bf16 ? 2 : 4), sbytes = (size_t)n_images * 3 * sizeof(double);
  LX_CHECK_ARG(!byte_ranges_overlap(x, xbytes, M, pbytes) && !byte_ranges_overlap(x, xbytes, sums, sbytes) &&
               !byte_ranges_overlap(x, xbytes, workspace, workspace_bytes),
               "%s: M, sums and the workspace may not overlap x[0, n_parts n)", name);
  if (int s = check_step_aliases(name, "x[0, n_parts n)", x, xbytes, v, !v_is_bf16, x0, z, m, pbytes)) return s;
  LX_CHECK_ARG(!byte_ranges_overlap(v, vbytes, M, pbytes), "%s: M may not overlap v (it is written while v is read)", name);
  if (ms)
    if (int s = check_multi_aliases(name, "x[0, n_parts n)", ms->D, x, xbytes, v, vbytes, x0, z, m, pbytes)) return s;
  LX_CHECK_ARG(!ms || (!byte_ranges_overlap(ms->D, pbytes, M, pbytes) && !byte_ranges_overlap(ms->D, pbytes, sums, sbytes) &&
                       !byte_ranges_overlap(ms->D, pbytes, workspace, workspace_bytes)),
               "%s: D may not overlap M, sums or the workspace", name);
  // every part and every image start: elems is the stride between them
  const Blend bl{x0, z, m, sigma_next, 1.0f - sigma_next};
  if (step_vec16(elems, addr_bits(x, M, x0, z, m, ms ? ms->D : nullptr), v, v_is_bf16))
    launch_apg<4>(x, v, v_is_bf16, n_parts, scale_a, scale_b, sigma, dsigma, eta, norm_threshold, momentum, M, sums, (double*)workspace, bl, n_images, elems, (hipStream_t)stream, ms);
  else launch_apg<1>(x, v, v_is_bf16, n_parts, scale_a, scale_b, sigma, dsigma, eta, norm_threshold, momentum, M, sums, (double*)workspace, bl, n_images, elems, (hipStream_t)stream, ms);
  LX_LAUNCH_CHECK(name);
  return LX_OK;
}

}  // namespace

// the unguided step stays on the element instantiation: moving the headline path onto 16-byte accesses would be a change of speed
extern "C" int lx_euler_step(float* x, const void* v, int v_is_bf16, float dsigma, size_t n, void* stream) {
  LX_CHECK_ARG(x && v, "lx_euler_step: NULL operand");
  if (n == 0) return LX_OK;
  launch_parts<1, 1, false>(x, v, v_is_bf16, dsigma, 0.f, 0.f, Blend{}, n, (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_euler_step");
  return LX_OK;
}

extern "C" int lx_scale_noise(float* out, const float* x0, const float* z, float sigma, size_t n, void* stream) {
  LX_CHECK_ARG(out && x0 && z, "lx_scale_noise: NULL operand");
  const size_t bytes = n * sizeof(float);
  LX_CHECK_ARG(!byte_ranges_overlap(out, bytes, x0, bytes) && !byte_ranges_overlap(out, bytes, z, bytes), "lx_scale_noise: x0 and z may not alias out");
  if (n == 0) return LX_OK;
  const float oms = 1.0f - sigma;
  if (step_vec16(0, addr_bits(out, x0, z), nullptr, 0))
    hipLaunchKernelGGL(scale_noise_kernel<4>, dim3(step_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, x0, z, sigma, oms, n);
  else hipLaunchKernelGGL(scale_noise_kernel<1>, dim3(step_grid(n)), dim3(256), 0, (hipStream_t)stream, out, x0, z, sigma, oms, n);
  LX_LAUNCH_CHECK("lx_scale_noise");
  return LX_OK;
}

extern "C" int lx_euler_step_blend(float* x, const void* v, int v_is_bf16, float dsigma, const float* x0, const float* z, const float* m,
                                   float sigma_next, size_t n, void* stream) {
  LX_CHECK_ARG(x && v && x0 && z && m, "lx_euler_step_blend: NULL operand");
  const size_t bytes = n * sizeof(float);
  if (int s = check_step_aliases("lx_euler_step_blend", "x", x, bytes, v, false, x0, z, m, bytes)) return s;
  if (n == 0) return LX_OK;
  // (not launch_step<1>: its instantiations without the blend would include a 16-byte unguided step that nothing launches)
  const Blend bl{x0, z, m, sigma_next, 1.0f - sigma_next};
  if (step_vec16(0, addr_bits(x, x0, z, m), v, v_is_bf16)) launch_parts<4, 1, true>(x, v, v_is_bf16, dsigma, 0.f, 0.f, bl, n, (hipStream_t)stream);
  else launch_parts<1, 1, true>(x, v, v_is_bf16, dsigma, 0.f, 0.f, bl, n, (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_euler_step_blend");
  return LX_OK;
}

extern "C" int lx_euler_step_cfg(float* x, const void* v, int v_is_bf16, float dsigma, float scale, const float* x0, const float* z,
                                 const float* m, float sigma_next, size_t n, void* stream) {
  LX_CHECK_ARG(x && v, "lx_euler_step_cfg: NULL x or v");
  LX_CHECK_ARG(n > 0, "lx_euler_step_cfg: n == 0");
  LX_CHECK_ARG(blend_triple_ok(x0, z, m), "lx_euler_step_cfg: x0, z and m go together (all NULL: no blend)");
  LX_CHECK_ARG(f32_is_finite(scale), "lx_euler_step_cfg: scale is not finite");
  if (int s = check_step_aliases("lx_euler_step_cfg", "x[0, 2n)", x, 2 * n * sizeof(float), v, !v_is_bf16, x0, z, m, n * sizeof(float))) return s;
  launch_step<2>(x, v, v_is_bf16, dsigma, scale, 0.f, x0, z, m, sigma_next, n, step_vec16(n, addr_bits(x, x0, z, m), v, v_is_bf16),
                 (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_euler_step_cfg");
  return LX_OK;
}

extern "C" int lx_euler_step_cfg3(float* x, const void* v, int v_is_bf16, float dsigma, float scale_brain, float scale_text, const float* x0,
                                  const float* z, const float* m, float sigma_next, size_t n, void* stream) {
  LX_CHECK_ARG(x && v, "lx_euler_step_cfg3: NULL x or v");
  LX_CHECK_ARG(n > 0, "lx_euler_step_cfg3: n == 0");
  LX_CHECK_ARG(n <= SIZE_MAX / (3 * sizeof(float)), "lx_euler_step_cfg3: 3n elements do not fit an address");
  LX_CHECK_ARG(blend_triple_ok(x0, z, m), "lx_euler_step_cfg3: x0, z and m go together (all NULL: no blend)");
  LX_CHECK_ARG(f32_is_finite(scale_brain) && f32_is_finite(scale_text), "lx_euler_step_cfg3: scale_brain or scale_text is not finite");
  if (int s = check_step_aliases("lx_euler_step_cfg3", "x[0, 3n)", x, 3 * n * sizeof(float), v, !v_is_bf16, x0, z, m, n * sizeof(float))) return s;
  launch_step<3>(x, v, v_is_bf16, dsigma, scale_brain, scale_text, x0, z, m, sigma_next, n,
                 step_vec16(n, addr_bits(x, x0, z, m), v, v_is_bf16), (hipStream_t)stream);
  LX_LAUNCH_CHECK("lx_euler_step_cfg3");
  return LX_OK;
}

extern "C" size_t lx_apg_workspace_bytes(int n_images, size_t elems) { return apg_workspace(n_images, elems); }

extern "C" int lx_euler_step_apg(float* x, const void* v, int v_is_bf16, int n_parts, float scale_a, float scale_b, float sigma, float dsigma,
                                 float eta, float norm_threshold, float momentum, float* M, double* sums, void* workspace,
                                 size_t workspace_bytes, const float* x0, const float* z, const float* m, float sigma_next, int n_images,
                                 size_t elems, void* stream) {
  return apg_entry("lx_euler_step_apg", x, v, v_is_bf16, n_parts, scale_a, scale_b, sigma, dsigma, nullptr, eta, norm_threshold, momentum, M,
                   sums, workspace, workspace_bytes, x0, z, m, sigma_next, n_images, elems, stream);
}

// ---- the second-order multistep step (DPM-Solver++(2M) on the flow's sigmas): the Euler entries above with one more term ------------------
extern "C" int lx_dpmpp2m_step(float* x, const void* v, int v_is_bf16, int n_parts, float scale_a, float scale_b, float sigma, float dsigma,
                               float c, float* D, const float* x0, const float* z, const float* m, float sigma_next, size_t n, void* stream) {
  LX_CHECK_ARG(x && v && D, "lx_dpmpp2m_step: NULL x, v or D");
  LX_CHECK_ARG(n_parts >= 1 && n_parts <= 3, "lx_dpmpp2m_step: n_parts=%d must be 1, 2 or 3", n_parts);
  LX_CHECK_ARG(n > 0, "lx_dpmpp2m_step: n == 0");
  LX_CHECK_ARG(n <= SIZE_MAX / (3 * sizeof(float)), "lx_dpmpp2m_step: 3n elements do not fit an address");
  LX_CHECK_ARG(f32_is_finite(sigma) && sigma > 0.f, "lx_dpmpp2m_step: sigma must be finite and > 0");
  LX_CHECK_ARG(f32_is_finite(c), "lx_dpmpp2m_step: c is not finite");
  LX_CHECK_ARG((n_parts < 2 || f32_is_finite(scale_a)) && (n_parts < 3 || f32_is_finite(scale_b)), "lx_dpmpp2m_step: a scale is not finite");
  LX_CHECK_ARG(blend_triple_ok(x0, z, m), "lx_dpmpp2m_step: x0, z and m go together (all NULL: no blend)");
  const size_t xbytes = (size_t)n_parts * n * sizeof(float), pbytes = n * sizeof(float), vbytes = (size_t)n_parts * n * (v_is_bf16 ? 2 : 4);
  if (int s = check_step_aliases("lx_dpmpp2m_step", "x[0, n_parts n)", x, xbytes, v, !v_is_bf16, x0, z, m, pbytes)) return s;
  if (int s = check_multi_aliases("lx_dpmpp2m_step", "x[0, n_parts n)", D, x, xbytes, v, vbytes, x0, z, m, pbytes)) return s;
  const Multi ms{D, c, -sigma};
  const bool vec = step_vec16(n_parts > 1 ? n : 0, addr_bits(x, x0, z, m, D), v, v_is_bf16);
  if (n_parts == 1) launch_step<1, true>(x, v, v_is_bf16, dsigma, 0.f, 0.f, x0, z, m, sigma_next, n, vec, (hipStream_t)stream, ms);
  else if (n_parts == 2) launch_step<2, true>(x, v, v_is_bf16, dsigma, scale_a, 0.f, x0, z, m, sigma_next, n, vec, (hipStream_t)stream, ms);
  else launch_step<3, true>(x, v, v_is_bf16, dsigma, scale_a, scale_b, x0, z, m, sigma_next, n, vec, (hipStream_t)stream, ms);
  LX_LAUNCH_CHECK("lx_dpmpp2m_step");
  return LX_OK;
}

extern "C" int lx_dpmpp2m_step_apg(float* x, const void* v, int v_is_bf16, int n_parts, float scale_a, float scale_b, float sigma, float dsigma,
                                   float c, float* D, float eta, float norm_threshold, float momentum, float* M, double* sums, void* workspace,
                                   size_t workspace_bytes, const float* x0, const float* z, const float* m, float sigma_next, int n_images,
                                   size_t elems, void* stream) {
  const Multi ms{D, c, -sigma};
  return apg_entry("lx_dpmpp2m_step_apg", x, v, v_is_bf16, n_parts, scale_a, scale_b, sigma, dsigma, &ms, eta, norm_threshold, momentum, M,
                   sums, workspace, workspace_bytes, x0, z, m, sigma_next, n_images, elems, stream);
}

// ---- FlowEdit (Kulikov et al.): the inputs of one forward on [target; source], and the update of the edit state after it -----------------
extern "C" int lx_flowedit_inputs(float* out, const float* x_src, const float* z_fe, const float* noise, float sigma, size_t n, void* stream) {
  LX_CHECK_ARG(out && x_src && z_fe && noise, "lx_flowedit_inputs: NULL operand");
  LX_CHECK_ARG(n > 0, "lx_flowedit_inputs: n == 0");
  LX_CHECK_ARG(n <= SIZE_MAX / (2 * sizeof(float)), "lx_flowedit_inputs: 2n elements do not fit an address");
  LX_CHECK_ARG(f32_is_finite(sigma) && sigma >= 0.f && sigma <= 1.f, "lx_flowedit_inputs: sigma must be finite and lie in [0, 1]");
  const size_t obytes = 2 * n * sizeof(float), pbytes = n * sizeof(float);
  LX_CHECK_ARG(!byte_ranges_overlap(out, obytes, x_src, pbytes) && !byte_ranges_overlap(out, obytes, z_fe, pbytes) &&
               !byte_ranges_overlap(out, obytes, noise, pbytes),
               "lx_flowedit_inputs: x_src, z_fe and noise may not overlap out[0, 2n)");
  const float oms = 1.0f - sigma;
  if (step_vec16(n, addr_bits(out, x_src, z_fe, noise), nullptr, 0))
    hipLaunchKernelGGL(flowedit_inputs_kernel<4>, dim3(step_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, out, x_src, z_fe, noise, sigma, oms, n);
  else hipLaunchKernelGGL(flowedit_inputs_kernel<1>, dim3(step_grid(n)), dim3(256), 0, (hipStream_t)stream, out, x_src, z_fe, noise, sigma, oms, n);
  LX_LAUNCH_CHECK("lx_flowedit_inputs");
  return LX_OK;
}

extern "C" int lx_flowedit_step(float* z_fe, const void* v, int v_is_bf16, float coef, const float* m, size_t n, void* stream) {
  LX_CHECK_ARG(z_fe && v, "lx_flowedit_step: NULL z_fe or v");
  LX_CHECK_ARG(n > 0, "lx_flowedit_step: n == 0");
  LX_CHECK_ARG(n <= SIZE_MAX / (2 * sizeof(float)), "lx_flowedit_step: 2n elements do not fit an address");
  LX_CHECK_ARG(f32_is_finite(coef), "lx_flowedit_step: coef is not finite");
  const size_t pbytes = n * sizeof(float);
  LX_CHECK_ARG(!byte_ranges_overlap(z_fe, pbytes, v, 2 * n * (v_is_bf16 ? 2 : 4)), "lx_flowedit_step: v may not overlap z_fe[0, n) (it is updated in place)");
  LX_CHECK_ARG(!m || !byte_ranges_overlap(z_fe, pbytes, m, pbytes), "lx_flowedit_step: m may not overlap z_fe[0, n) (it is updated in place)");
  const bool vec = step_vec16(n, addr_bits(z_fe, m), v, v_is_bf16);
  const dim3 grid(step_grid(vec ? n / 4 : n));
  if (vec && m) hipLaunchKernelGGL((flowedit_step_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, z_fe, v, v_is_bf16, coef, m, n);
  else if (vec) hipLaunchKernelGGL((flowedit_step_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, z_fe, v, v_is_bf16, coef, m, n);
  else if (m) hipLaunchKernelGGL((flowedit_step_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)stream, z_fe, v, v_is_bf16, coef, m, n);
  else hipLaunchKernelGGL((flowedit_step_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)stream, z_fe, v, v_is_bf16, coef, m, n);
  LX_LAUNCH_CHECK("lx_flowedit_step");
  return LX_OK;
}
