// Attack-step kernels (gfx950): everything the update rules of pgd.py launch between two gradient
// passes — the pixel-gradient assembly, the sign / L2 / momentum / TI / DI / SI / VT / SPSA / UAP /
// APGD / SignHunter / PI updates, C&W, Adam and the patch update. Images are fp32 NCHW planes.
#include "attack_common.h"

namespace mia {

template <typename T>
__global__ void image_grad_kernel(const float* __restrict__ rec, const float* __restrict__ t,
                                  const T* __restrict__ gv, float* __restrict__ gimg, int N, int S,
                                  int pf, int cpad, float coef) {
  const int R = S / pf;
  const int64_t total = (int64_t)N * 3 * S * S;
  const float inv = 1.f / (float)(pf * pf);
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int x = (int)(i % S);
    const int y = (int)((i / S) % S);
    const int c = (int)((i / ((int64_t)S * S)) % 3);
    const int n = (int)(i / ((int64_t)S * S * 3));
    float g = coef * (rec[i] - t[i]);
    if (gv) g += to_f(gv[(((size_t)n * R + y / pf) * R + x / pf) * cpad + c]) * inv;
    gimg[i] = g;
  }
}

// ---------------------------------------------------------------------------------------------
// K11: PGD step with cost = −L (interpolation.py:92-94; torchattacks targeted form :83-86).
// Every operation is a single fp32 op with no contraction opportunity (a·sign is exact), so for an
// identical gradient the result is bit-identical to torch's fp32 CPU ops.
__device__ __forceinline__ float project1(float xa, float x0, float g, float a, float e, float lo,
                                          float hi) {
#pragma clang fp contract(off)
  const float sg = g < 0.f ? 1.f : (g > 0.f ? -1.f : 0.f);  // sign(−g)
  float adv = xa + a * sg;
  float d = adv - x0;
  d = fminf(fmaxf(d, -e), e);
  float r = x0 + d;
  return fminf(fmaxf(r, lo), hi);
}

__global__ void random_start_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                    const float* __restrict__ u, int64_t len, float e, float lo,
                                    float hi) {
#pragma clang fp contract(off)
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float ue = e * u[i];  // rounded separately (no contraction), as torch mul then add
    x[i] = fminf(fmaxf(x0[i] + ue, lo), hi);
  }
}

__global__ void sign_project_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                    const float* __restrict__ g, int64_t len, float a, float e,
                                    float lo, float hi) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB)
    x[i] = project1(x[i], x0[i], g[i], a, e, lo, hi);
}

// ∇_x L at image element i (NCHW fp32, S² planes): the image-MSE term coef_img·(x − x0) plus the
// adjoints of the two avg_pool2d's (attack_main2.py:590-591): the VGG input-path gradient at S/pf
// (NHWC, cpad channels) and the encoder gradient at enc_res, each spread over its pooling window.
template <typename T>
__device__ __forceinline__ float assemble_grad(int64_t i, float xv, float x0v, const T* gv,
                                               const float* genc, int S, int pf, int cpad,
                                               int enc_res, float coef_img) {
  const int R = S / pf;
  const int ek = S / enc_res;
  const int xx = (int)(i % S);
  const int yy = (int)((i / S) % S);
  const int c = (int)((i / ((int64_t)S * S)) % 3);
  const int n = (int)(i / ((int64_t)S * S * 3));
  float g = coef_img * (xv - x0v);
  if (gv) g += to_f(gv[(((size_t)n * R + yy / pf) * R + xx / pf) * cpad + c]) / (float)(pf * pf);
  if (genc) g += genc[(((size_t)n * 3 + c) * enc_res + yy / ek) * enc_res + xx / ek] / (float)(ek * ek);
  return g;
}

// A non-finite gradient element (an fp16 loss-scale overflow upstream, or a NaN in the
// weights) marks its image in nonfinite[n]; the host reads the flags once per attack
// (pgd.AttackEngine) instead of letting sign(NaN) = 0 freeze the pixel silently. Racing writers
// store the same value.
__device__ __forceinline__ void flag_nonfinite(int* nonfinite, int64_t i, int S, float g) {
  if (nonfinite && !__builtin_isfinite(g)) nonfinite[i / ((int64_t)3 * S * S)] = 1;
}

template <typename T>
__global__ void pgd_update_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                  const T* __restrict__ gv, const float* __restrict__ genc, int N,
                                  int S, int pf, int cpad, int enc_res, float coef_img, float a,
                                  float e, float lo, float hi, int* __restrict__ nonfinite) {
  const int64_t total = (int64_t)N * 3 * S * S;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const float xv = x[i], x0v = x0[i];
    const float g = assemble_grad(i, xv, x0v, gv, genc, S, pf, cpad, enc_res, coef_img);
    flag_nonfinite(nonfinite, i, S, g);
    x[i] = project1(xv, x0v, g, a, e, lo, hi);
  }
}

template <typename T>
__global__ void grad_assemble_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                     const T* __restrict__ gv, const float* __restrict__ genc,
                                     float* __restrict__ g, int N, int S, int pf, int cpad,
                                     int enc_res, float coef_img, float scale,
                                     int* __restrict__ nonfinite) {
  const int64_t total = (int64_t)N * 3 * S * S;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const float v = scale * assemble_grad(i, x[i], x0[i], gv, genc, S, pf, cpad, enc_res, coef_img);
    flag_nonfinite(nonfinite, i, S, v);
    g[i] = v;
  }
}

// ---- L2-ball PGD (torchattacks PGDL2) and momentum iterative FGSM (torchattacks MIFGSM) --------
// Both need a per-image norm of the pixel gradient, so the gradient is materialised once
// (grad_assemble_norms_kernel, with its Σ|g| and Σg²) and the updates read the norm from device
// memory. Every kernel here runs on a (slots, N) grid, block (b, n) striding over image n alone
// (attack_common.h: ldv / stv, lane_sum, block_slot_store).

// g = scale·∇_x L (grad_assemble_kernel's expression: the same bits) with the per-image partial
// sums of |g| (quantity 0) and g² (quantity 1).
template <typename T, int V>
__global__ __launch_bounds__(TPB) void grad_assemble_norms_kernel(
    const float* __restrict__ x, const float* __restrict__ x0, const T* __restrict__ gv,
    const float* __restrict__ genc, float* __restrict__ g, float* __restrict__ part, int64_t plane,
    int S, int pf, int cpad, int enc_res, float coef_img, float scale,
    int* __restrict__ nonfinite) {
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, nv = plane / V;
  float a1[V], a2[V];
#pragma unroll
  for (int e = 0; e < V; ++e) a1[e] = a2[e] = 0.f;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < nv; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * V;
    float xv[V], x0v[V], o[V];
    ldv<V>(x + i0, xv);
    ldv<V>(x0 + i0, x0v);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float v =
          scale * assemble_grad(i0 + e, xv[e], x0v[e], gv, genc, S, pf, cpad, enc_res, coef_img);
      if (nonfinite && !__builtin_isfinite(v)) nonfinite[n] = 1;
      o[e] = v;
      a1[e] += fabsf(v);
      a2[e] += v * v;
    }
    stv<V>(g + i0, o);
  }
  block_slot_store<2>(lane_sum<V>(a1), lane_sum<V>(a2), part);
}

// torchattacks PGDL2.forward, the ascent half, on cost = −L:
//   adv = x + a·((−g) / (‖g_n‖₂ + 1e-10)),  ‖g_n‖₂ = sqrt(gnorm2sq[n])
// written to x un-projected, with the per-image partial sums of (adv − x0)². One fp32 rounding
// per operation (IEEE division and square root, no contraction), as torch's fp32 CPU ops.
template <int V>
__global__ __launch_bounds__(TPB) void l2_step_kernel(float* __restrict__ x,
                                                      const float* __restrict__ x0,
                                                      const float* __restrict__ g,
                                                      const float* __restrict__ gnorm2sq,
                                                      float* __restrict__ part, int64_t plane,
                                                      float a, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, nv = plane / V;
  const float gn = sqrtf(gnorm2sq[n]) + 1e-10f;
  if (nonfinite && threadIdx.x == 0 && !__builtin_isfinite(gn)) nonfinite[n] = 1;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < nv; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * V;
    float xv[V], x0v[V], gg[V];
    ldv<V>(x + i0, xv);
    ldv<V>(x0 + i0, x0v);
    ldv<V>(g + i0, gg);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float t = (-gg[e]) / gn;
      if (nonfinite && !__builtin_isfinite(t)) nonfinite[n] = 1;
      const float s = a * t;
      const float adv = xv[e] + s;
      const float d = adv - x0v[e];
      const float dd = d * d;
      acc[e] += dd;
      xv[e] = adv;
    }
    stv<V>(x + i0, xv);
  }
  block_slot_store<1>(lane_sum<V>(acc), 0.f, part);
}

// torchattacks PGDL2.forward, the projection half: d = x − x0; f = min(e / ‖d_n‖₂, 1)
// (e / 0 = +inf → 1); x = clamp(x0 + d·f, lo, hi), ‖d_n‖₂ = sqrt(dsq[n]).
template <int V>
__global__ __launch_bounds__(TPB) void l2_project_kernel(float* __restrict__ x,
                                                         const float* __restrict__ x0,
                                                         const float* __restrict__ dsq,
                                                         int64_t plane, float e, float lo,
                                                         float hi) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, nv = plane / V;
  const float dn = sqrtf(dsq[n]);
  const float f = fminf(e / dn, 1.f);
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < nv; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * V;
    float xv[V], x0v[V];
    ldv<V>(x + i0, xv);
    ldv<V>(x0 + i0, x0v);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = xv[k] - x0v[k];
      const float df = d * f;
      const float r = x0v[k] + df;
      xv[k] = fminf(fmaxf(r, lo), hi);
    }
    stv<V>(x + i0, xv);
  }
}

// torchattacks MIFGSM.forward on cost = −L, one pass:
//   ĝ = (−g) / (l1[n] / plane);  m = ĝ + μ·m;
//   x = clamp(x0 + clamp(x + a·sign(m) − x0, −e, e), lo, hi)
// One fp32 rounding per operation. A non-finite ĝ (zero or non-finite mean, 0/0) marks the image.
template <int V>
__global__ __launch_bounds__(TPB) void mi_update_kernel(float* __restrict__ x,
                                                        const float* __restrict__ x0,
                                                        const float* __restrict__ g,
                                                        const float* __restrict__ l1,
                                                        float* __restrict__ m, int64_t plane,
                                                        float mu, float a, float e, float lo,
                                                        float hi, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, nv = plane / V;
  const float mean = l1[n] / (float)plane;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < nv; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * V;
    float xv[V], x0v[V], gg[V], mv[V];
    ldv<V>(x + i0, xv);
    ldv<V>(x0 + i0, x0v);
    ldv<V>(g + i0, gg);
    ldv<V>(m + i0, mv);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float gh = (-gg[k]) / mean;
      if (nonfinite && !__builtin_isfinite(gh)) nonfinite[n] = 1;
      const float dec = mu * mv[k];
      const float mm = gh + dec;
      mv[k] = mm;
      const float sg = mm > 0.f ? 1.f : (mm < 0.f ? -1.f : 0.f);
      const float adv = xv[k] + a * sg;
      float d = adv - x0v[k];
      d = fminf(fmaxf(d, -e), e);
      const float r = x0v[k] + d;
      xv[k] = fminf(fmaxf(r, lo), hi);
    }
    stv<V>(m + i0, mv);
    stv<V>(x + i0, xv);
  }
}

// ---- scale-invariant and Nesterov attacks (torchattacks SINIFGSM / NIFGSM). Both kernels run on
// the (slots, N) grid above, but a thread always owns one GROUP of 4 consecutive elements of its
// image (the last group of a plane that is no multiple of 4 is partial): VEC moves the group as
// one 16-byte vector, !VEC as guarded scalars. The grid and the element → accumulator mapping are
// the same either way, so the two forms give the same bits, sums included.
template <bool VEC>
__device__ __forceinline__ void ld4(const float* __restrict__ p, int cnt, float (&v)[4]) {
  if (VEC) {
    ldv<4>(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < cnt ? p[e] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void st4(float* __restrict__ p, int cnt, const float (&v)[4]) {
  if (VEC) {
    stv<4>(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) p[e] = v[e];
  }
}

// The input of scale copy i at the Nesterov look-ahead point:
//   t = m ? x + c·m : x  (c = μ·a);   y = s == 1 ? t : (t + 1)·s − 1  (s = 2^-i)
// — torchattacks' p / 2^i on p = (x + 1)/2 ∈ [0,1], written in [-1,1] units: towards black. One
// fp32 rounding per operation; not clamped (as torchattacks). m = nullptr and s = 1: a bit copy.
template <bool VEC>
__global__ __launch_bounds__(TPB) void si_transform_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ m,
                                                           float* __restrict__ y, int64_t plane,
                                                           float c, float s) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.y * plane, ng = (plane + 3) / 4;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float v[4];
    ld4<VEC>(x + i0, cnt, v);
    if (m) {
      float mv[4];
      ld4<VEC>(m + i0, cnt, mv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float look = c * mv[e];
        v[e] = v[e] + look;
      }
    }
    if (s != 1.f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = v[e] + 1.f;
        const float ps = p * s;
        v[e] = ps - 1.f;
      }
    }
    st4<VEC>(y + i0, cnt, v);
  }
}

// One scale copy's gradient into the step's accumulator:
//   v = w·g (w = 2^-i: exact);  r = first ? v : acc + v;  div ≠ 1: r = r / div (IEEE);  acc = r
// with the per-image partial sums of |r| (quantity 0) and r² (quantity 1). The engine passes
// div = the number of copies on the last one only. One fp32 rounding per operation; r² enters
// its sum through an fma, unrounded.
template <bool VEC>
__global__ __launch_bounds__(TPB) void si_accumulate_norms_kernel(
    const float* __restrict__ g, float* __restrict__ acc, float* __restrict__ part, int64_t plane,
    float w, int first, float div, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, ng = (plane + 3) / 4;
  float a1[4], a2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = a2[e] = 0.f;
  bool bad = false;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float r[4];
    ld4<VEC>(g + i0, cnt, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = w * r[e];
    if (!first) {
      float av[4];
      ld4<VEC>(acc + i0, cnt, av);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = av[e] + r[e];
    }
    if (div != 1.f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = r[e] / div;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // the lanes past a partial group hold 0
      bad |= !__builtin_isfinite(r[e]);
      a1[e] += fabsf(r[e]);
      a2[e] = fmaf(r[e], r[e], a2[e]);
    }
    st4<VEC>(acc + i0, cnt, r);
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<2>(lane_sum<4>(a1), lane_sum<4>(a2), part);
}

// ---- variance-tuned attacks (torchattacks VMIFGSM; Wang & He's VNI with the look-ahead). Both
// kernels run on the SI kernels' (slots, N) grid, a thread owning one group of 4 consecutive
// elements of its image, so VEC and the guarded scalars give the same bits. The neighbours' noise
// is counter-based and stateless: Philox4x32-10 (Salmon et al., Random123) keyed with the attack's
// seed, the counter (group index within the image, GLOBAL image index, step, sample). One block
// of 4 words is exactly one group's noise, so an element's value depends on nothing else: not on
// the batch, the grid, the vector form or the rank that holds the image.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;  // the Weyl sequence of the key
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// One neighbour of the (look-ahead) iterate:
//   t = m ? x + c·m : x  (as si_transform_kernel);  y = t + r·u,
//   u = float(2·(bits >> 8) + 1 − 2^24)·2^-24: an odd integer below 2^24 times 2^-24, exact in
// fp32, symmetric in (−1, 1), never 0 or ±1. One fp32 rounding per operation; not clamped.
template <bool VEC>
__global__ __launch_bounds__(TPB) void vt_neighbor_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ m,
                                                          float* __restrict__ y, int64_t plane,
                                                          float c, float r, uint32_t k0,
                                                          uint32_t k1, uint32_t image0,
                                                          uint32_t step, uint32_t sample) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.y * plane, ng = (plane + 3) / 4;
  const uint32_t image = image0 + blockIdx.y;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float v[4];
    ld4<VEC>(x + i0, cnt, v);
    if (m) {
      float mv[4];
      ld4<VEC>(m + i0, cnt, mv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float look = c * mv[e];
        v[e] = v[e] + look;
      }
    }
    uint32_t b[4];
    philox4x32_10((uint32_t)j, image, step, sample, k0, k1, b);  // j < 2^29
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float u = (float)((int)(2u * (b[e] >> 8) + 1u) - (1 << 24)) * 0x1p-24f;
      const float ru = r * u;
      v[e] = v[e] + ru;
    }
    st4<VEC>(y + i0, cnt, v);
  }
}

// The tuned gradient and the next variance term in one pass:
//   gt = g + v (the OLD v), with the per-image partial sums of |gt|;  gv ? v = gv − g : v stays.
// One fp32 rounding per operation; the lanes past a partial group hold 0.
template <bool VEC>
__global__ __launch_bounds__(TPB) void vt_combine_norms_kernel(
    const float* __restrict__ g, const float* __restrict__ gv, float* __restrict__ v,
    float* __restrict__ gt, float* __restrict__ part, int64_t plane,
    int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, ng = (plane + 3) / 4;
  float a1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = 0.f;
  bool bad = false;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float gg[4], vv[4], t[4];
    ld4<VEC>(g + i0, cnt, gg);
    ld4<VEC>(v + i0, cnt, vv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t[e] = gg[e] + vv[e];
      bad |= !__builtin_isfinite(t[e]);
      a1[e] += fabsf(t[e]);
    }
    st4<VEC>(gt + i0, cnt, t);
    if (gv) {
      float nv[4];
      ld4<VEC>(gv + i0, cnt, nv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        nv[e] = nv[e] - gg[e];
        bad |= !__builtin_isfinite(nv[e]);
      }
      st4<VEC>(v + i0, cnt, nv);
    }
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<1>(lane_sum<4>(a1), 0.f, part);
}

// ---- SPSA (Spall 1992; Uesato et al. 2018; torchattacks SPSA's estimator), a score-based
// black-box attack: the gradient is estimated from objective VALUES at antithetic probes
// x ± d·v, v Rademacher. Both kernels run on the VT kernels' (slots, N) grid, a thread owning one
// group of 4 consecutive elements of its image = one Philox block, counter (group index, GLOBAL
// image index, step, sample): the directions are never stored, the accumulation regenerates them.
// v = +1 where bit 31 of the element's word is 0, −1 where it is 1.
//
// The two probes of one pair in one pass (one read of x, one Philox block):
//   t = v > 0 ? d : −d;  yp = clamp(x + t, lo, hi);  ym = clamp(x − t, lo, hi)
// One fp32 rounding per operation.
template <bool VEC>
__global__ __launch_bounds__(TPB) void spsa_probe_kernel(const float* __restrict__ x,
                                                         float* __restrict__ yp,
                                                         float* __restrict__ ym, int64_t plane,
                                                         float d, float lo, float hi, uint32_t k0,
                                                         uint32_t k1, uint32_t image0,
                                                         uint32_t step, uint32_t sample) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.y * plane, ng = (plane + 3) / 4;
  const uint32_t image = image0 + blockIdx.y;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float v[4], p[4], q[4];
    ld4<VEC>(x + i0, cnt, v);
    uint32_t b[4];
    philox4x32_10((uint32_t)j, image, step, sample, k0, k1, b);  // j < 2^29
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = (b[e] >> 31) ? -d : d;
      const float up = v[e] + t;
      const float dn = v[e] - t;
      p[e] = fminf(fmaxf(up, lo), hi);
      q[e] = fminf(fmaxf(dn, lo), hi);
    }
    st4<VEC>(yp + i0, cnt, p);
    st4<VEC>(ym + i0, cnt, q);
  }
}

// One pair's term into the step's estimate, with the per-image norms of the result:
//   c = (fp[n] − fm[n])·s;  t = v > 0 ? c : −c;  r = first ? t : acc + t;
//   div ≠ 1: r = r / div (IEEE);  acc = r
// with the per-image partial sums of |r| (quantity 0) and r² (quantity 1), as
// si_accumulate_norms_kernel. One fp32 rounding per operation; r² enters its sum through an fma,
// unrounded. A non-finite objective reaches every r of its image through c.
template <bool VEC>
__global__ __launch_bounds__(TPB) void spsa_accumulate_norms_kernel(
    float* __restrict__ acc, const float* __restrict__ fp, const float* __restrict__ fm,
    float* __restrict__ part, int64_t plane, float s, uint32_t k0, uint32_t k1, uint32_t image0,
    uint32_t step, uint32_t sample, int first, float div, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, ng = (plane + 3) / 4;
  const uint32_t image = image0 + blockIdx.y;
  const float df = fp[n] - fm[n];
  const float c = df * s;
  float a1[4], a2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = a2[e] = 0.f;
  bool bad = false;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    uint32_t b[4];
    philox4x32_10((uint32_t)j, image, step, sample, k0, k1, b);  // j < 2^29
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = e < cnt ? ((b[e] >> 31) ? -c : c) : 0.f;
    if (!first) {
      float av[4];
      ld4<VEC>(acc + i0, cnt, av);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = av[e] + r[e];
    }
    if (div != 1.f) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = r[e] / div;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // the lanes past a partial group hold 0
      bad |= !__builtin_isfinite(r[e]);
      a1[e] += fabsf(r[e]);
      a2[e] = fmaf(r[e], r[e], a2[e]);
    }
    st4<VEC>(acc + i0, cnt, r);
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<2>(lane_sum<4>(a1), lane_sum<4>(a2), part);
}

// ---- Universal perturbation: ONE δ plane for all images, updated from the sign of an exact
// integer sum over the images. Both kernels run on a 1-D grid over the groups of 4 consecutive
// plane elements (VEC / guarded scalars as above: the same bits); the thread that owns a group
// walks the images, UAP_UNROLL loads in flight.
typedef long long i64x2 __attribute__((ext_vector_type(2)));
constexpr int UAP_UNROLL = 8;
constexpr float UAP_ONE = 16777216.f;  // 2^24, the fixed point of the per-image terms

template <bool VEC>
__device__ __forceinline__ void ld4i(const long long* __restrict__ p, int cnt, long long (&v)[4]) {
  if (VEC) {
    const i64x2 a = *(const i64x2*)p, b = *(const i64x2*)(p + 2);
    v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < cnt ? p[e] : 0;
  }
}

// Per image n and element j:  ĝ = (−g) / (l1[n] / plane)  (mia_mi_update's normalisation, the same
// bits);  q = (int64) rint(ĝ·2^24)  (the product is exact, rint is round-half-even, and the result
// is an integer fp32 holds exactly);  acc_j = (first ? 0 : acc_j) + Σ_n q_n,j.
// |ĝ| < 2·plane is the range the caller's bound rests on: an element outside it (NaN and ±Inf
// included) marks its image and contributes 0. Integer sums are associative, so neither the order
// of the images nor the split over calls, blocks or ranks can change a bit. gridDim.y = 1: the
// thread owns its group and stores it. gridDim.y > 1 (the image-split form, MIA_UAP_SPLIT): block
// row y sums a contiguous share of the images and adds it with 64-bit vector integer atomics to an
// acc the launcher zeroed when first.
template <bool VEC>
__global__ __launch_bounds__(TPB) void uap_accumulate_kernel(
    const float* __restrict__ g, const float* __restrict__ l1, long long* __restrict__ acc, int N,
    int64_t plane, int first, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int64_t ng = (plane + 3) / 4;
  const float fplane = (float)plane, lim = 2.f * fplane;
  const int share = (N + (int)gridDim.y - 1) / (int)gridDim.y;
  const int n_lo = (int)blockIdx.y * share, n_hi = n_lo + share < N ? n_lo + share : N;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = j * 4;
    const int cnt = (int)(plane - i0 < 4 ? plane - i0 : 4);
    long long s[4] = {0, 0, 0, 0};
    for (int n0 = n_lo; n0 < n_hi; n0 += UAP_UNROLL) {
      float v[UAP_UNROLL][4], mean[UAP_UNROLL];
#pragma unroll
      for (int u = 0; u < UAP_UNROLL; ++u)
        if (n0 + u < n_hi) {
          ld4<VEC>(g + (int64_t)(n0 + u) * plane + i0, cnt, v[u]);
          mean[u] = l1[n0 + u] / fplane;
        }
#pragma unroll
      for (int u = 0; u < UAP_UNROLL; ++u)
        if (n0 + u < n_hi) {
          bool bad = false;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float gh = (-v[u][e]) / mean[u];
            const bool ok = fabsf(gh) < lim;  // false for NaN
            bad |= !ok && e < cnt;
            const float p = gh * UAP_ONE;
            s[e] += ok ? (long long)__builtin_rintf(p) : 0LL;
          }
          if (bad && nonfinite) nonfinite[n0 + u] = 1;
        }
    }
    if (gridDim.y > 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) atomicAdd((unsigned long long*)(acc + i0 + e), (unsigned long long)s[e]);
      continue;
    }
    if (!first) {
      long long old[4];
      ld4i<VEC>(acc + i0, cnt, old);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += old[e];
    }
    if (VEC) {
      i64x2 a, b;
      a[0] = s[0], a[1] = s[1], b[0] = s[2], b[1] = s[3];
      *(i64x2*)(acc + i0) = a;
      *(i64x2*)(acc + i0 + 2) = b;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) acc[i0 + e] = s[e];
    }
  }
}

// δ_j ← clamp(δ_j + a·sgn(acc_j), −e, e)  (sgn(0) = 0; acc = nullptr: δ is only read), then for
// every image x_n,j = clamp(x0_n,j + δ_j, lo, hi), in one pass. One fp32 rounding per operation
// (a·sgn is exact). N = 0: δ only.
template <bool VEC>
__global__ __launch_bounds__(TPB) void uap_step_kernel(float* __restrict__ delta,
                                                       const long long* __restrict__ acc,
                                                       float* __restrict__ x,
                                                       const float* __restrict__ x0, int N,
                                                       int64_t plane, float a, float e, float lo,
                                                       float hi) {
#pragma clang fp contract(off)
  const int64_t ng = (plane + 3) / 4;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = j * 4;
    const int cnt = (int)(plane - i0 < 4 ? plane - i0 : 4);
    float d[4];
    ld4<VEC>(delta + i0, cnt, d);
    if (acc) {
      long long A[4];
      ld4i<VEC>(acc + i0, cnt, A);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float sg = A[k] > 0 ? 1.f : (A[k] < 0 ? -1.f : 0.f);
        const float s = a * sg;
        const float t = d[k] + s;
        d[k] = fminf(fmaxf(t, -e), e);
      }
      st4<VEC>(delta + i0, cnt, d);
    }
    for (int n0 = 0; n0 < N; n0 += UAP_UNROLL) {
      float v[UAP_UNROLL][4];
#pragma unroll
      for (int u = 0; u < UAP_UNROLL; ++u)
        if (n0 + u < N) ld4<VEC>(x0 + (int64_t)(n0 + u) * plane + i0, cnt, v[u]);
#pragma unroll
      for (int u = 0; u < UAP_UNROLL; ++u)
        if (n0 + u < N) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float r = v[u][k] + d[k];
            v[u][k] = fminf(fmaxf(r, lo), hi);
          }
          st4<VEC>(x + (int64_t)(n0 + u) * plane + i0, cnt, v[u]);
        }
    }
  }
}

// ---- Auto-PGD (Croce & Hein 2020; torchattacks APGD.attack_single_run, norm = 'Linf') on
// cost = −L. Three kernels per step. The update and the copies run on the SI kernels' (slots, N)
// grid, a thread owning one group of 4 consecutive elements of its image, so VEC and the guarded
// scalars give the same bits. Per-image state is only ever READ by those two (eta, action); it is
// written by the decision kernel, one thread per image, in a launch of its own — no block reads
// what another block of its launch rewrites.
//
// The momentum step with a per-image step size eta[n], torchattacks' bound form:
//   d = x − x_old;  x_old = x
//   z = clamp(min(max(x − eta[n]·sign(g), x0 − e), x0 + e), lo, hi)
//   x = clamp(min(max((x + (z − x)·a) + d·(1 − a), x0 − e), x0 + e), lo, hi)
// One fp32 rounding per operation (1 − a too); sign(0) = sign(NaN) = 0.
template <bool VEC>
__global__ __launch_bounds__(TPB) void apgd_update_kernel(float* __restrict__ x,
                                                          float* __restrict__ x_old,
                                                          const float* __restrict__ x0,
                                                          const float* __restrict__ g,
                                                          const float* __restrict__ eta,
                                                          int64_t plane, float a, float e, float lo,
                                                          float hi, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * plane, ng = (plane + 3) / 4;
  const float step = eta[n];
  const float b = 1.f - a;
  bool bad = false;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float xv[4], ov[4], x0v[4], gg[4];
    ld4<VEC>(x + i0, cnt, xv);
    ld4<VEC>(x_old + i0, cnt, ov);
    ld4<VEC>(x0 + i0, cnt, x0v);
    ld4<VEC>(g + i0, cnt, gg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // the lanes past a partial group hold 0 and are not stored
      bad |= !__builtin_isfinite(gg[k]);
      const float d = xv[k] - ov[k];
      ov[k] = xv[k];
      const float sg = gg[k] > 0.f ? 1.f : (gg[k] < 0.f ? -1.f : 0.f);
      const float lb = x0v[k] - e;
      const float ub = x0v[k] + e;
      const float t = xv[k] - step * sg;  // eta·(±1 | 0) is exact
      const float z = fminf(fmaxf(fminf(fmaxf(t, lb), ub), lo), hi);
      const float zx = z - xv[k];
      const float za = zx * a;
      const float s1 = xv[k] + za;
      const float db = d * b;
      const float s2 = s1 + db;
      xv[k] = fminf(fmaxf(fminf(fmaxf(s2, lb), ub), lo), hi);
    }
    st4<VEC>(x_old + i0, cnt, ov);
    st4<VEC>(x + i0, cnt, xv);
  }
  if (bad && nonfinite) nonfinite[n] = 1;
}

// Per-image state of the step-size control: fs = fp32 (4, N) rows eta, L_best, L_prev, L_check;
// is = int32 (3, N) rows n_dec, reduced, best_step.
enum { APGD_ETA = 0, APGD_LBEST = 1, APGD_LPREV = 2, APGD_LCHECK = 3 };
enum { APGD_NDEC = 0, APGD_REDUCED = 1, APGD_BESTSTEP = 2 };

// One thread per image. step = 0, the start: the state is initialised from L(x) and eta0, and the
// action is SAVE. step = i + 1, after update i: with L = loss[n],
//   L < L_prev: n_dec += 1;  L_prev = L;  L < L_best: L_best = L, best_step = step, SAVE
//   at a checkpoint: flag = n_dec <= thr || (reduced == 0 && L_check <= L_best);
//                    reduced = flag;  L_check = L_best;  n_dec = 0;  flag: eta /= 2, RESTORE
// A NaN objective fails every comparison: never a decrease, never the best. The row (L, eta) is
// appended to the history.
__global__ void apgd_decide_kernel(const float* __restrict__ loss, float* __restrict__ fs,
                                   int* __restrict__ is, int* __restrict__ action,
                                   float* __restrict__ hist_loss, float* __restrict__ hist_eta,
                                   int N, int step, int checkpoint, int thr, float eta0) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float L = loss[n];
  float eta;
  int act = 0;
  if (step == 0) {
    eta = eta0;
    fs[APGD_LBEST * N + n] = L;
    fs[APGD_LPREV * N + n] = L;
    fs[APGD_LCHECK * N + n] = L;
    is[APGD_NDEC * N + n] = 0;
    is[APGD_REDUCED * N + n] = 1;
    is[APGD_BESTSTEP * N + n] = 0;
    act = MIA_APGD_SAVE;
  } else {
    eta = fs[APGD_ETA * N + n];
    float best = fs[APGD_LBEST * N + n];
    int ndec = is[APGD_NDEC * N + n];
    if (L < fs[APGD_LPREV * N + n]) ++ndec;
    fs[APGD_LPREV * N + n] = L;
    if (L < best) {
      best = L;
      fs[APGD_LBEST * N + n] = L;
      is[APGD_BESTSTEP * N + n] = step;
      act |= MIA_APGD_SAVE;
    }
    if (checkpoint) {
      const bool flag = ndec <= thr ||
                        (is[APGD_REDUCED * N + n] == 0 && fs[APGD_LCHECK * N + n] <= best);
      is[APGD_REDUCED * N + n] = flag ? 1 : 0;
      fs[APGD_LCHECK * N + n] = best;
      ndec = 0;
      if (flag) {
        eta = eta / 2.f;
        act |= MIA_APGD_RESTORE;
      }
    }
    is[APGD_NDEC * N + n] = ndec;
  }
  fs[APGD_ETA * N + n] = eta;
  action[n] = act;
  hist_loss[n] = L;
  hist_eta[n] = eta;
}

// The whole-image copies the decision asked for, per image n (action[n] was written by an earlier
// launch): SAVE: x_best = x, g_best = g;  RESTORE without SAVE: x = x_best, g = g_best. With both
// bits the best point IS the iterate, so the restore is the identity and only the save runs.
template <bool VEC>
__global__ __launch_bounds__(TPB) void apgd_apply_kernel(float* __restrict__ x,
                                                         float* __restrict__ g,
                                                         float* __restrict__ x_best,
                                                         float* __restrict__ g_best,
                                                         const int* __restrict__ action,
                                                         int64_t plane) {
  const int act = action[blockIdx.y];
  if (!(act & (MIA_APGD_SAVE | MIA_APGD_RESTORE))) return;
  const bool save = act & MIA_APGD_SAVE;
  const float* sx = save ? x : x_best;
  const float* sg = save ? g : g_best;
  float* dx = save ? x_best : x;
  float* dg = save ? g_best : g;
  const int64_t base = (int64_t)blockIdx.y * plane, ng = (plane + 3) / 4;
  for (int64_t j = blockIdx.x * (int64_t)TPB + threadIdx.x; j < ng; j += (int64_t)gridDim.x * TPB) {
    const int64_t i0 = base + j * 4;
    const int cnt = (int)(plane - j * 4 < 4 ? plane - j * 4 : 4);
    float v[4], w[4];
    ld4<VEC>(sx + i0, cnt, v);
    ld4<VEC>(sg + i0, cnt, w);
    st4<VEC>(dx + i0, cnt, v);
    st4<VEC>(dg + i0, cnt, w);
  }
}

// ---- SignHunter (Al-Dujaili & O'Reilly 2020): every iterate is a vertex clamp(x0 + e·s) of the
// ball, s ∈ {−1, +1} stored as int8 (a clamped element of x no longer shows its sign). A query
// flips s on one contiguous segment [lo, hi) of every image and, in the same pass, flips the
// previous query's segment [plo, phi) back in the images whose decision (accept[n], written by an
// EARLIER launch of sh_decide_kernel) rejected it:
//   m = (plo ≤ j < phi && accept[n] == 0 ? −1 : 1)·(lo ≤ j < hi ? −1 : 1)
//   j in either range:  s[j] *= m;  x[j] = clamp(x0[j] + e·s[j], lo_v, hi_v)
// e·s is ±e exactly, so x is one fp32 rounding. The grid covers the groups g0 … g0 + ng − 1 of 4
// consecutive elements (counted from the image start) that the hull of the two ranges meets; a
// thread owns one group and masks its lanes: an element outside both ranges is neither loaded nor
// stored, one inside their union is written exactly once. VEC moves a group that lies wholly
// inside the union as one 16-byte (x, x0) / 4-byte (s) vector and every other group as guarded
// scalars, !VEC all of them as scalars: the same bits.
template <bool VEC>
__global__ __launch_bounds__(TPB) void sh_flip_kernel(float* __restrict__ x,
                                                      const float* __restrict__ x0,
                                                      signed char* __restrict__ s,
                                                      const int* __restrict__ accept,
                                                      int64_t plane, int64_t g0, int64_t ng,
                                                      int64_t plo, int64_t phi, int64_t lo,
                                                      int64_t hi, float e, float lo_v, float hi_v) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  const bool revert = accept != nullptr && accept[n] == 0;
  const int64_t base = (int64_t)n * plane;
  for (int64_t t = blockIdx.x * (int64_t)TPB + threadIdx.x; t < ng; t += (int64_t)gridDim.x * TPB) {
    const int64_t j0 = (g0 + t) * 4;
    bool on[4], neg[4];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t j = j0 + k;
      const bool ip = j >= plo && j < phi, in = j >= lo && j < hi;
      on[k] = ip || in;
      neg[k] = (ip && revert) != in;
      cnt += on[k] ? 1 : 0;
    }
    if (cnt == 0) continue;
    const int64_t i0 = base + j0;
    if (VEC && cnt == 4) {
      float xv[4], x0v[4];
      ldv<4>(x0 + i0, x0v);
      const char4 sv = *reinterpret_cast<const char4*>(s + i0);
      signed char sk[4] = {(signed char)sv.x, (signed char)sv.y, (signed char)sv.z,
                           (signed char)sv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (neg[k]) sk[k] = (signed char)-sk[k];
        const float r = x0v[k] + (sk[k] < 0 ? -e : e);
        xv[k] = fminf(fmaxf(r, lo_v), hi_v);
      }
      *reinterpret_cast<char4*>(s + i0) = make_char4(sk[0], sk[1], sk[2], sk[3]);
      stv<4>(x + i0, xv);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!on[k]) continue;
        signed char sk = s[i0 + k];
        if (neg[k]) sk = (signed char)-sk;
        const float r = x0[i0 + k] + (sk < 0 ? -e : e);
        s[i0 + k] = sk;
        x[i0 + k] = fminf(fmaxf(r, lo_v), hi_v);
      }
    }
  }
}

// The accept / reject decision of one query, one thread per image, on L = loss[n]:
//   first (query 0): best = L, accept = 1, n_accept = 0
//   else:            accept = L < best;  accept: best = L, n_accept += 1
// A tie, a NaN and ±Inf are rejections; a non-finite L marks its image. hist_loss[n] = L.
__global__ void sh_decide_kernel(const float* __restrict__ loss, float* __restrict__ best,
                                 int* __restrict__ accept, int* __restrict__ n_accept,
                                 float* __restrict__ hist_loss, int N, int first,
                                 int* __restrict__ nonfinite) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float L = loss[n];
  const bool finite = __builtin_isfinite(L);
  if (!finite && nonfinite) nonfinite[n] = 1;
  if (first) {
    best[n] = L;
    accept[n] = 1;
    n_accept[n] = 0;
  } else {
    const bool acc = finite && L < best[n];
    if (acc) {
      best[n] = L;
      n_accept[n] += 1;
    }
    accept[n] = acc ? 1 : 0;
  }
  hist_loss[n] = L;
}

// ---- translation-invariant smoothing (torchattacks TIFGSM): gs = (taps ⊗ taps) ⋆ g per plane,
// zero padded, with the per-image partial sums of |gs| (quantity 0) and gs² (quantity 1).
// One block = one TI_T × TI_T output tile of one plane, on a (C·tiles, N) grid: the geometry
// depends on (C, H, W) only. Three phases over LDS:
//   A  the tile with its halo (zero outside the plane), r = K/2 rows above / below and
//      rl = r rounded up to 4 columns left / right, so that a 16-byte global vector is whole;
//   B  the horizontal pass over every row of A;
//   the vertical pass over B, into registers, stored with the sums.
// Every output is t[0]·v[0] followed by fma(t[k], v[k], ·) for k = 1 … K−1 in both passes: its
// value depends on its plane and position only, never on the tile layout or the batch. The taps
// are staged in LDS and read as uniform 16-byte vectors, 8 taps per loop trip.
// LDS banking: A's row stride is odd, so the 4 rows × 8 column groups that a 32-lane half reads
// in the horizontal pass (ds_read_b32, bank = dword mod 32) fall on 32 distinct banks, and so do
// the vector path's stores; B's rows are 64 dwords, written and read as whole 16-byte slots.
constexpr int TI_T = 64;     // tile edge
constexpr int TI_MAXK = 63;  // largest kernel
constexpr int TI_OFFA = 68;  // LDS floats [0, 68): 3 unused, the taps, zeros up to a whole vector

struct TiGeom {
  int r, rl, HA, WA, SA, offB, floats;
  __host__ __device__ explicit TiGeom(int K) {
    r = K >> 1;
    rl = (r + 3) & ~3;
    HA = TI_T + K - 1;
    WA = TI_T + 2 * rl;
    SA = WA + 3;  // odd; the passes prefetch up to 2 elements / rows past their last operand
    offB = (TI_OFFA + HA * SA + 3) & ~3;
    floats = offB + (HA + 2) * TI_T;
  }
};

__device__ __forceinline__ float ti_fma(float t, float v, float acc) { return fmaf(t, v, acc); }
__device__ __forceinline__ f32x4 ti_fma(float t, f32x4 v, f32x4 acc) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaf(t, v[e], acc[e]);
  return o;
}

// Taps k … k + 2·NP − 1 (k ≡ 1 mod 8, tk = &taps[k], 16-byte aligned) added to the 4 outputs
// acc[o] = Σ t[j]·in[o + j]; in[j] = *(T*)(src + j·stride) lives in w[j & 7]. On entry w holds
// in[k … k + 4]; every pair of taps first fetches the two inputs that the NEXT pair adds.
template <typename T, int NP>
__device__ __forceinline__ void ti_pairs(const float* __restrict__ src, int stride, int k,
                                         const float* __restrict__ tk, T (&w)[8], T (&acc)[4]) {
  float tv[8];
#pragma unroll
  for (int j = 0; j < (2 * NP + 3) / 4; ++j) {
    const f32x4 v = *(const f32x4*)(tk + 4 * j);
#pragma unroll
    for (int e = 0; e < 4; ++e) tv[4 * j + e] = v[e];
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    constexpr int ph = 1;  // k & 7
    const int kk = ph + 2 * p;
    w[(kk + 5) & 7] = *(const T*)(src + (k + 2 * p + 5) * stride);
    w[(kk + 6) & 7] = *(const T*)(src + (k + 2 * p + 6) * stride);
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[o] = ti_fma(tv[2 * p], w[(kk + o) & 7], acc[o]);
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[o] = ti_fma(tv[2 * p + 1], w[(kk + 1 + o) & 7], acc[o]);
  }
}

// acc[o] = Σ_{j<K} t[j]·in[o + j] for o = 0 … 3 in tap order (K odd: tap 0, then pairs); reads up
// to in[K + 4], two past the last operand. tapS[3 + j] = t[j].
template <typename T>
__device__ __forceinline__ void ti_filter(const float* __restrict__ src, int stride,
                                          const float* __restrict__ tapS, int K, T (&acc)[4]) {
  T w[8];
#pragma unroll
  for (int j = 0; j < 6; ++j) w[j] = *(const T*)(src + j * stride);
  const float t0 = tapS[3];
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = t0 * w[o];
  int k = 1;
  for (; k + 8 <= K; k += 8) ti_pairs<T, 4>(src, stride, k, tapS + 3 + k, w, acc);
  switch ((K - k) >> 1) {
    case 1: ti_pairs<T, 1>(src, stride, k, tapS + 3 + k, w, acc); break;
    case 2: ti_pairs<T, 2>(src, stride, k, tapS + 3 + k, w, acc); break;
    case 3: ti_pairs<T, 3>(src, stride, k, tapS + 3 + k, w, acc); break;
    default: break;
  }
}

template <int V>
__global__ __launch_bounds__(TPB) void ti_smooth_norms_kernel(
    const float* __restrict__ g, float* __restrict__ gs, const float* __restrict__ taps, int K,
    float* __restrict__ part, int C, int H, int W, int tiles_x, int tiles_y,
    int* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) float ti_lds[];
  const TiGeom q(K);
  const int r = q.r, rl = q.rl, HA = q.HA, WA = q.WA, SA = q.SA;
  float* __restrict__ A = ti_lds + TI_OFFA;
  float* __restrict__ B = ti_lds + q.offB;
  const int t = threadIdx.x, n = blockIdx.y;
  const int tiles = tiles_x * tiles_y;
  const int c = blockIdx.x / tiles, tile = blockIdx.x - c * tiles;
  const int ty0 = (tile / tiles_x) * TI_T, tx0 = (tile % tiles_x) * TI_T;
  const int64_t pbase = ((int64_t)n * C + c) * ((int64_t)H * W);
  const float* __restrict__ gp = g + pbase;

  if (t < TI_OFFA) ti_lds[t] = t >= 3 && t - 3 < K ? taps[t - 3] : 0.f;
  if (V == 4) {
    // 32 consecutive items = 4 rows × 8 vectors: conflict-free dword stores at the odd stride
    const int NC = WA >> 2, NCB = (NC + 7) >> 3, items = ((HA + 3) >> 2) * NCB * 32;
#pragma unroll 2
    for (int i = t; i < items; i += TPB) {
      const int l = i & 31, b = i >> 5;
      const int cc = (b % NCB) * 8 + (l & 7), row = (b / NCB) * 4 + (l >> 3);
      if (cc < NC && row < HA) {
        const int gy = ty0 - r + row, gx = tx0 - rl + 4 * cc;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const f32x4*)(gp + gy * W + gx);
        float* a = A + row * SA + 4 * cc;
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = v[e];
      }
    }
  } else {
    for (int i = t; i < HA * WA; i += TPB) {
      const int row = i / WA, col = i - row * WA;
      const int gy = ty0 - r + row, gx = tx0 - rl + col;
      A[row * SA + col] = gy >= 0 && gy < H && gx >= 0 && gx < W ? gp[gy * W + gx] : 0.f;
    }
  }
  __syncthreads();

  // horizontal pass: 4 adjacent outputs of one row of A per thread
  {
    const int lane = t & 63, wv = t >> 6;
    const int xg = (lane & 7) + 8 * (wv & 1);
    for (int row = (lane >> 3) + 8 * (wv >> 1); row < HA; row += 16) {
      float h[4];
      ti_filter<float>(A + row * SA + (rl - r) + 4 * xg, 1, ti_lds, K, h);
      const f32x4 o4 = {h[0], h[1], h[2], h[3]};
      *(f32x4*)(B + row * TI_T + 4 * xg) = o4;
    }
  }
  __syncthreads();

  // vertical pass: a 4 × 4 patch per thread down 4 columns of B, the same tap order
  const int x4 = (t & 15) * 4, y0 = (t >> 4) * 4;
  f32x4 acc[4];
  ti_filter<f32x4>(B + y0 * TI_T + x4, TI_T, ti_lds, K, acc);

  float s1 = 0.f, s2 = 0.f;
  bool bad = false;
  float* __restrict__ op = gs + pbase;
  const int gx = tx0 + x4;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int gy = ty0 + y0 + o;
    if (gy >= H) break;
    if (V == 4) {
      if (gx < W) {  // W % 4 == 0: the vector is whole
        *(f32x4*)(op + gy * W + gx) = acc[o];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[o][e];
          bad |= !__builtin_isfinite(v);
          s1 += fabsf(v);
          s2 = fmaf(v, v, s2);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gx + e < W) {
          const float v = acc[o][e];
          op[gy * W + gx + e] = v;
          bad |= !__builtin_isfinite(v);
          s1 += fabsf(v);
          s2 = fmaf(v, v, s2);
        }
    }
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<2>(s1, s2, part);
}

// ---- the patch-wise attack (Gao et al., "Patch-wise Attack for Fooling Deep Neural Network",
// ECCV 2020; PI-FGSM): the MIFGSM step amplified to ab = β·a, with the part of the accumulated
// noise A that overflows the ε-ball handed to each pixel's neighbours instead of clipped away.
// Per plane and pixel, one fp32 rounding per line, no contraction:
//   ĝ  = (−g) / (l1[n] / plane);  m' = ĝ + μ·m;  s = sign(m')      (mi_update_kernel's, same bits)
//   A' = A + ab·s;  C = sign(A')·max(|A'| − e, 0)                  (the cut noise, 0 in the ball)
//   S  = Σ_{dy = −r … r} Σ_{dx = −r … r, (dy, dx) ≠ (0, 0)} C[y + dy, x + dx]
//        (additions from 0, dy outer and dx inner, both ascending; zero outside the plane)
//   p  = gm·sign(S);  A ← A' + p
//   u  = x + ab·s;  v = u + p;  x ← clamp(x0 + clamp(v − x0, −e, e), lo, hi);  m ← m'
// Only sign(S) is used, so the uniform project kernel's weight 1/(K² − 1) drops out and S is a
// chain of plain additions in a fixed order: its value depends on the plane and the position
// only, never on the tile layout or the batch.
// One block = one TI_T × TI_T tile of one plane on a (C·tiles, N) grid, as ti_smooth_norms_kernel;
// a thread owns a 4 × 4 patch (4 adjacent columns of 4 rows). Phase 1 computes m', A' and C of
// the patch (kept in registers) and C of the halo ring — r rows above / below, rl = r rounded up
// to 4 columns left / right, so that a 16-byte vector is whole — into LDS; an element outside the
// plane is never read and its C is 0. Phase 2 walks the K + 3 LDS rows under the patch once, each
// as whole 16-byte slots, and adds row j to the window row dy = j − o of output row o. m and A are
// read from m_in / A_in and written to m_out / A_out: a block's halo reads its neighbours' OLD
// state while they write the new one. x is in place (only the thread's own elements are read).
// VEC (W % 4 == 0, 16-byte aligned bases) moves the 4 columns as one vector, the scalar form the
// same elements of the same thread one by one: the same bits.
constexpr int PI_MAXK = 15;  // largest project kernel

template <int K>
struct PiGeom {
  static constexpr int r = K >> 1;
  static constexpr int rl = (r + 3) & ~3;
  static constexpr int HA = TI_T + 2 * r;
  static constexpr int WA = TI_T + 2 * rl;
  static constexpr int SA = WA + 4;  // rows stay 16-byte aligned; rows 8 apart are 32 banks apart
  static constexpr int floats = HA * SA;
};

__device__ __forceinline__ float pi_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// m' (mm), A' (ap) and the cut noise C (returned) of one element; bad |= a non-finite ĝ
__device__ __forceinline__ float pi_cut(float g, float m, float A, float mean, float mu, float ab,
                                        float e, float& mm, float& ap, bool& bad) {
#pragma clang fp contract(off)
  const float gh = (-g) / mean;
  bad |= !__builtin_isfinite(gh);
  const float dec = mu * m;
  mm = gh + dec;
  const float st = ab * pi_sign(mm);
  ap = A + st;
  const float over = fmaxf(fabsf(ap) - e, 0.f);
  return ap > 0.f ? over : (ap < 0.f ? -over : 0.f);
}

template <int K, bool VEC>
__global__ __launch_bounds__(TPB) void pi_update_kernel(
    float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
    const float* __restrict__ l1, const float* __restrict__ m_in, float* __restrict__ m_out,
    const float* __restrict__ A_in, float* __restrict__ A_out, int C, int H, int W, int tiles_x,
    int tiles_y, float mu, float ab, float gm, float e, float lo, float hi,
    int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  typedef PiGeom<K> Q;
  constexpr int r = Q::r, rl = Q::rl, SA = Q::SA, NC = Q::WA / 4;
  __shared__ __attribute__((aligned(16))) float cut[Q::floats];
  const int t = threadIdx.x, n = blockIdx.y;
  const int tiles = tiles_x * tiles_y;
  const int c = blockIdx.x / tiles, tile = blockIdx.x - c * tiles;
  const int ty0 = (tile / tiles_x) * TI_T, tx0 = (tile % tiles_x) * TI_T;
  const int64_t hw = (int64_t)H * W;
  const int64_t pbase = ((int64_t)n * C + c) * hw;
  const float mean = l1[n] / (float)((int64_t)C * hw);

  // phase 1, the thread's own patch: rows ty0 + y0 + o, columns gx … gx + 3, cnt[o] of them inside
  const int x4 = (t & 15) * 4, y0 = (t >> 4) * 4;
  const int gx = tx0 + x4;
  float mm[4][4], ap[4][4];
  int cnt[4];
  bool bad = false;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int gy = ty0 + y0 + o;
    cnt[o] = gy < H && gx < W ? (W - gx < 4 ? W - gx : 4) : 0;
    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
    if (cnt[o] > 0) {
      const int64_t i0 = pbase + (int64_t)gy * W + gx;
      float gg[4], mv[4], av[4];
      ld4<VEC>(g + i0, cnt[o], gg);
      ld4<VEC>(m_in + i0, cnt[o], mv);
      ld4<VEC>(A_in + i0, cnt[o], av);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt[o]) cv[k] = pi_cut(gg[k], mv[k], av[k], mean, mu, ab, e, mm[o][k], ap[o][k], bad);
    }
    *(f32x4*)(cut + (r + y0 + o) * SA + rl + x4) = cv;
  }
  if (bad && nonfinite) nonfinite[n] = 1;

  // phase 1, the halo ring in 4-column slots: the r rows above and below over the whole width,
  // then the rl / 4 slots left and right of each of the TI_T rows
  {
    constexpr int NTB = 2 * r * NC, NSV = rl / 2, NRING = NTB + TI_T * NSV;
    for (int i = t; i < NRING; i += TPB) {
      int row, col4;
      if (i < NTB) {
        row = i / NC;
        col4 = i - row * NC;
        if (row >= r) row += TI_T;
      } else {
        const int j = i - NTB, rr = j / NSV, cs = j - rr * NSV;
        row = r + rr;
        col4 = cs < rl / 4 ? cs : cs + TI_T / 4;
      }
      const int hy = ty0 - r + row, hx = tx0 - rl + 4 * col4;
      const int hc = hy >= 0 && hy < H && hx >= 0 && hx < W ? (W - hx < 4 ? W - hx : 4) : 0;
      f32x4 cv = {0.f, 0.f, 0.f, 0.f};
      if (hc > 0) {
        const int64_t i0 = pbase + (int64_t)hy * W + hx;
        float gg[4], mv[4], av[4];
        ld4<VEC>(g + i0, hc, gg);
        ld4<VEC>(m_in + i0, hc, mv);
        ld4<VEC>(A_in + i0, hc, av);
        bool unused = false;
        float mh, ah;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < hc) cv[k] = pi_cut(gg[k], mv[k], av[k], mean, mu, ab, e, mh, ah, unused);
      }
      *(f32x4*)(cut + row * SA + 4 * col4) = cv;
    }
  }
  __syncthreads();

  // phase 2: LDS row y0 + j lies under window row dy = j − o of the patch's output row o
  float S[4][4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int k = 0; k < 4; ++k) S[o][k] = 0.f;
  const float* __restrict__ src = cut + y0 * SA + x4;
#pragma unroll 1
  for (int j = 0; j < K + 3; ++j) {
    float w[4 + 2 * rl];
#pragma unroll
    for (int q = 0; q < 1 + rl / 2; ++q) {
      const f32x4 v = *(const f32x4*)(src + j * SA + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) w[4 * q + k] = v[k];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int dy = j - o;
      if (dy < 0 || dy >= K) continue;
      if (dy == r) {
#pragma unroll
        for (int dx = 0; dx < K; ++dx)
          if (dx != r)
#pragma unroll
            for (int k = 0; k < 4; ++k) S[o][k] += w[rl - r + k + dx];
      } else {
#pragma unroll
        for (int dx = 0; dx < K; ++dx)
#pragma unroll
          for (int k = 0; k < 4; ++k) S[o][k] += w[rl - r + k + dx];
      }
    }
  }

#pragma unroll
  for (int o = 0; o < 4; ++o) {
    if (cnt[o] == 0) continue;
    const int64_t i0 = pbase + (int64_t)(ty0 + y0 + o) * W + gx;
    float xv[4], x0v[4], mo[4], ao[4];
    ld4<VEC>(x + i0, cnt[o], xv);
    ld4<VEC>(x0 + i0, cnt[o], x0v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt[o]) continue;
      const float p = gm * pi_sign(S[o][k]);
      ao[k] = ap[o][k] + p;
      mo[k] = mm[o][k];
      const float st = ab * pi_sign(mm[o][k]);
      const float u = xv[k] + st;
      const float v = u + p;
      float d = v - x0v[k];
      d = fminf(fmaxf(d, -e), e);
      const float rr = x0v[k] + d;
      xv[k] = fminf(fmaxf(rr, lo), hi);
    }
    st4<VEC>(x + i0, cnt[o], xv);
    st4<VEC>(m_out + i0, cnt[o], mo);
    st4<VEC>(A_out + i0, cnt[o], ao);
  }
}

// ---- input diversity (torchattacks DIFGSM / TIFGSM input_diversity at a fixed image size) ------
// y = D(x): every plane resized bilinearly (align_corners = False) to rnd × rnd and placed at
// (top, left) of a zero S × S plane; gx = Dᵀ g with the per-image partial sums of |gx| and gx².
// The source of output o along one axis is an exact rational: n = (2o+1)·S − rnd over d = 2·rnd,
//   i0 = n / d,  i1 = min(i0 + 1, S − 1),  w1 = λ = float(n − i0·d) / float(d),
//   w0 = float(d − (n − i0·d)) / float(d)
// (unsigned 32-bit: n < 2·S² < 2^32 because S² < 2^31; each weight is one IEEE division of two
// integers below 2^24, so w0 carries one rounding too instead of the two of 1 − λ). rnd ≤ S puts
// every source coordinate in [0, S − 1], and i0 = S − 1 only with λ = 0.
// A term whose weight is exactly 0 is left out and the sums start from −0, so rnd = S (every
// λ = 0, every w0 = 1) returns its input bit for bit. No contraction: products and additions
// round separately, forward  w0y·(w0x·a00 + w1x·a01) + w1y·(w0x·a10 + w1x·a11).
//
// Both kernels run one block per DI_TX × DI_TY tile of one plane on a (C·tiles, N) grid, a thread
// on 4 adjacent columns of DI_TY / 4 rows (row = wave + 4·k, wave-uniform): the geometry depends
// on (C, S) only. The per-column and per-row taps of the tile are worked out once per block into
// LDS (one integer division pair per tap instead of per element); VEC moves the 4 columns as one
// 16-byte vector (S % 4 == 0, aligned bases), the scalar form moves the same elements of the same
// thread one by one: the same bits, sums included.
constexpr int DI_TX = 256;  // tile columns: 64 lanes × 4
constexpr int DI_TY = 32;   // tile rows: 4 waves × 8

// forward tap of output o ∈ [0, rnd): source index i0 and the weights of i0 and i0 + 1
__device__ __forceinline__ void di_src(uint32_t o, uint32_t S, uint32_t rnd, int& i0, float& w0,
                                       float& w1) {
#pragma clang fp contract(off)
  const uint32_t d = 2u * rnd;
  const uint32_t n = (2u * o + 1u) * S - rnd;
  const uint32_t q = n / d, r = n - q * d;
  i0 = (int)q;
  w0 = (float)(d - r) / (float)d;
  w1 = (float)r / (float)d;
}

// adjoint tap of input i: the one output o with i0(o) == i (source coordinates are ≥ 1 apart, so
// there is at most one), or o = −1. i0(o) = i ⟺ (2i+1)·rnd ≤ (2o+1)·S < (2i+3)·rnd: the
// candidate is the smallest o that meets the left inequality, kept if the forward rule maps it to
// i. Input i then receives w0(o)·g[o] from this tap and w1(o')·g[o'] from the tap of i − 1.
__device__ __forceinline__ void di_adj(int i, int S, int rnd, int& o, float& w0, float& w1) {
  o = -1;
  w0 = w1 = 0.f;
  if (i < 0 || i >= S) return;
  const uint32_t a = (2u * (uint32_t)i + 1u) * (uint32_t)rnd;  // < 2·S²
  const uint32_t c = a <= (uint32_t)S ? 0u : (a + (uint32_t)S - 1u) / (2u * (uint32_t)S);
  if (c >= (uint32_t)rnd) return;
  int i0;
  float f0, f1;
  di_src(c, S, rnd, i0, f0, f1);
  if (i0 != i) return;
  o = (int)c;
  w0 = f0;
  w1 = f1;
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void di_resize_pad_kernel(const float* __restrict__ x,
                                                            float* __restrict__ y, int C, int S,
                                                            int rnd, int top, int left,
                                                            int tiles_x, int tiles_y) {
#pragma clang fp contract(off)
  __shared__ int si[DI_TX + DI_TY];  // columns of the tile, then its rows; −1 outside the window
  __shared__ float sw0[DI_TX + DI_TY], sw1[DI_TX + DI_TY];
  const int t = threadIdx.x, n = blockIdx.y;
  const int tiles = tiles_x * tiles_y;
  const int c = blockIdx.x / tiles, tile = blockIdx.x - c * tiles;
  const int ry0 = (tile / tiles_x) * DI_TY, cx0 = (tile % tiles_x) * DI_TX;
  for (int j = t; j < DI_TX + DI_TY; j += TPB) {
    const int o = j < DI_TX ? cx0 + j - left : ry0 + (j - DI_TX) - top;
    int i0 = -1;
    float w0 = 0.f, w1 = 0.f;
    if (o >= 0 && o < rnd) di_src(o, S, rnd, i0, w0, w1);
    si[j] = i0;
    sw0[j] = w0;
    sw1[j] = w1;
  }
  __syncthreads();
  const int lane = t & 63, wv = t >> 6;
  const int x0 = cx0 + 4 * lane;
  if (x0 >= S) return;
  const int64_t pbase = ((int64_t)n * C + c) * ((int64_t)S * S);
  const float* __restrict__ xp = x + pbase;
  float* __restrict__ yp = y + pbase;
  int ix[4];
  float wx0[4], wx1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ix[e] = si[4 * lane + e];
    wx0[e] = sw0[4 * lane + e];
    wx1[e] = sw1[4 * lane + e];
  }
  for (int k = 0; k < DI_TY / 4; ++k) {
    const int yy = ry0 + wv + 4 * k;
    if (yy >= S) break;
    const int jy = DI_TX + wv + 4 * k;
    const int iy = si[jy];
    const float wy0 = sw0[jy], wy1 = sw1[jy];
    float o4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = 0.f;
      if (iy >= 0 && ix[e] >= 0) {
        const bool hx = wx1[e] > 0.f, hy = wy1 > 0.f;
        const float* __restrict__ r0 = xp + (int64_t)iy * S;
        const float* __restrict__ r1 = xp + (int64_t)min(iy + 1, S - 1) * S;
        const int i0 = ix[e], i1 = min(ix[e] + 1, S - 1);
        const float t0 = wx0[e] * r0[i0];
        const float u0 = hx ? wx1[e] * r0[i1] : -0.f;
        const float s0 = t0 + u0;
        float s1 = -0.f;
        if (hy) {
          const float t1 = wx0[e] * r1[i0];
          const float u1 = hx ? wx1[e] * r1[i1] : -0.f;
          s1 = wy1 * (t1 + u1);
        }
        v = wy0 * s0 + s1;
      }
      o4[e] = v;
    }
    float* __restrict__ dst = yp + (int64_t)yy * S + x0;
    if (VEC) {
      stv<4>(dst, o4);  // S % 4 == 0: the vector is whole
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x0 + e < S) dst[e] = o4[e];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void di_resize_pad_bwd_norms_kernel(
    const float* __restrict__ g, float* __restrict__ gx, float* __restrict__ part, int C, int S,
    int rnd, int top, int left, int tiles_x, int tiles_y, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  // adjoint taps of columns cx0 − 1 … cx0 + DI_TX − 1, then of rows ry0 − 1 … ry0 + DI_TY − 1
  constexpr int NT = DI_TX + 1 + DI_TY + 1;
  __shared__ int so[NT];
  __shared__ float sw0[NT], sw1[NT];
  const int t = threadIdx.x, n = blockIdx.y;
  const int tiles = tiles_x * tiles_y;
  const int c = blockIdx.x / tiles, tile = blockIdx.x - c * tiles;
  const int ry0 = (tile / tiles_x) * DI_TY, cx0 = (tile % tiles_x) * DI_TX;
  for (int j = t; j < NT; j += TPB) {
    const int i = j <= DI_TX ? cx0 - 1 + j : ry0 - 1 + (j - DI_TX - 1);
    di_adj(i, S, rnd, so[j], sw0[j], sw1[j]);
  }
  __syncthreads();
  const int lane = t & 63, wv = t >> 6;
  const int x0 = cx0 + 4 * lane;
  const int64_t pbase = ((int64_t)n * C + c) * ((int64_t)S * S);
  const float* __restrict__ gp = g + pbase + (int64_t)top * S + left;  // the window's origin
  float* __restrict__ op = gx + pbase;
  float a1[4], a2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = a2[e] = 0.f;
  bool bad = false;
  if (x0 < S) {
    // column x0 − 1 + k: its output ox[k]; it gives column x0 − 1 + k weight wa[k] and column
    // x0 + k weight wb[k]
    int ox[5];
    float wa[5], wb[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      ox[k] = so[4 * lane + k];
      wa[k] = sw0[4 * lane + k];
      wb[k] = sw1[4 * lane + k];
    }
    for (int k = 0; k < DI_TY / 4; ++k) {
      const int yy = ry0 + wv + 4 * k;
      if (yy >= S) break;
      const int jy = DI_TX + 1 + wv + 4 * k;  // the tap of row yy − 1; jy + 1: of row yy
      const int oyB = so[jy], oyA = so[jy + 1];
      const float wyB = sw1[jy], wyA = sw0[jy + 1];
      const bool hB = oyB >= 0 && wyB > 0.f, hA = oyA >= 0;
      float vB[5], vA[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        vB[j] = hB && ox[j] >= 0 ? gp[(int64_t)oyB * S + ox[j]] : 0.f;
        vA[j] = hA && ox[j] >= 0 ? gp[(int64_t)oyA * S + ox[j]] : 0.f;
      }
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // oy ascending (B before A), then ox ascending (the tap of column − 1 first)
        const bool xB = ox[e] >= 0 && wb[e] > 0.f, xA = ox[e + 1] >= 0;
        const float pB0 = xB ? wb[e] * vB[e] : -0.f;
        const float pB1 = xA ? wa[e + 1] * vB[e + 1] : -0.f;
        const float pA0 = xB ? wb[e] * vA[e] : -0.f;
        const float pA1 = xA ? wa[e + 1] * vA[e + 1] : -0.f;
        const float sB = pB0 + pB1, sA = pA0 + pA1;
        const float qB = hB ? wyB * sB : -0.f;
        const float qA = hA ? wyA * sA : -0.f;
        const float v = (xB || xA) && (hB || hA) ? qB + qA : 0.f;
        o4[e] = v;
        if (VEC || x0 + e < S) {
          bad |= !__builtin_isfinite(v);
          a1[e] += fabsf(v);
          a2[e] = fmaf(v, v, a2[e]);
        }
      }
      float* __restrict__ dst = op + (int64_t)yy * S + x0;
      if (VEC) {
        stv<4>(dst, o4);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x0 + e < S) dst[e] = o4[e];
      }
    }
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<2>(lane_sum<4>(a1), lane_sum<4>(a2), part);
}

// ---- C&W L2 in tanh space (torchattacks CW, interpolation.py:98-193), images in [-1, 1]:
// adv = tanh(w) (= 2·½(tanh w + 1) − 1), w0 = atanh(x) with x clamped to ±(1 − 2⁻²⁰) so that
// saturated pixels stay finite.
__global__ void cw_init_kernel(const float* __restrict__ x, float* __restrict__ w, int64_t len) {
  constexpr float lim = 1.f - 9.5367431640625e-07f;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB)
    w[i] = atanhf(fminf(fmaxf(x[i], -lim), lim));
}

__global__ void cw_tanh_kernel(const float* __restrict__ w, float* __restrict__ adv, int64_t len) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB)
    adv[i] = tanhf(w[i]);
}

// ∂cost/∂w with cost = Σ_n ‖(adv − x)/2‖² + c·Σ_n f_n(adv) and adv = tanh w:
//   gw = (½(adv − x) + c·scale·g_f)·(1 − adv²)        (g_f = ∇f, loss-scaled; scale undoes it)
__global__ void cw_grad_kernel(const float* __restrict__ adv, const float* __restrict__ x,
                               const float* __restrict__ gf, float* __restrict__ gw, int64_t len,
                               float c, float scale) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float a = adv[i];
    gw[i] = (0.5f * (a - x[i]) + c * scale * gf[i]) * (1.f - a * a);
  }
}

// Best-L2 bookkeeping (torchattacks CW :154-163), one block per image: an image is a success when
// its objective is below the clean image's (f_n < f0_n, the GAN objective has no labels) and its
// L2 = l2_scale·Σ(adv − x)² beats the best so far; then best_adv[n] ← adv[n].
__global__ void cw_select_kernel(const float* __restrict__ adv, float* __restrict__ best_adv,
                                 const float* __restrict__ sq, float* __restrict__ best_l2,
                                 const float* __restrict__ f, const float* __restrict__ f0,
                                 int64_t plane, float l2_scale) {
  const int n = blockIdx.x;
  const float l2 = l2_scale * sq[n];
  const bool take = f[n] < f0[n] && best_l2[n] > l2;
  __syncthreads();
  if (!take) return;
  for (int64_t i = threadIdx.x; i < plane; i += TPB) best_adv[(size_t)n * plane + i] = adv[(size_t)n * plane + i];
  if (threadIdx.x == 0) best_l2[n] = l2;
}

// K12: Adam on pixels (torch.optim.Adam single-tensor semantics, no weight decay).
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t len, float lr, float b1, float b2,
                            float eps, float bc1, float bc2sqrt) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float gi = g[i];
    const float mi = m[i] + (1.f - b1) * (gi - m[i]);
    const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2sqrt + eps;
    p[i] = p[i] - (lr / bc1) * (mi / denom);
  }
}

// Adversarial patch (code/attack/patch/adversarial_patch.py:131-134, attack_main2.py:413-420):
//   patch −= g (the full-image gradient, step 1);  adv = (1 − m)·img + m·patch;
//   adv = clamp(adv, lo, hi) with lo / hi = min / max of the clean images.
// Each torch op is one fp32 rounding (no contraction), so the result is bit-identical to torch's
// fp32 ops for the same gradient. `g` may be null (composite only, patch_white_box). `shared` =
// numel of mask / patch when they are one image broadcast over the batch (0: same shape as img).
__global__ void patch_update_kernel(float* __restrict__ patch, const float* __restrict__ g,
                                    const float* __restrict__ img, const float* __restrict__ mask,
                                    float* __restrict__ adv, int64_t len, int64_t shared, float lo,
                                    float hi) {
#pragma clang fp contract(off)
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const int64_t j = shared ? i % shared : i;
    float pv = patch[j];
    if (g) {
      pv = pv - g[i];
      patch[j] = pv;
    }
    const float m = mask[j];
    const float a = (1.f - m) * img[i];
    const float b = m * pv;
    adv[i] = fminf(fmaxf(a + b, lo), hi);
  }
}

}  // namespace mia

using namespace mia;

// ---- what the launchers share ------------------------------------------------------------------
// A launcher reads: argument checks, the vec decision, the grid, one launch statement.

// (slots, N) grid of the per-image passes: ≤ 1024 slots of TPB threads, each moving V floats
static inline dim3 image_grid(int64_t plane, int V, int N) {
  return dim3(blocks_for(plane / V, TPB, 1024), N);
}

// The counter-based launchers (VT, SPSA): the 64-bit seed as Philox's two key words, and the
// image counters image0 … image0 + N − 1 within 32 bits.
struct PhiloxKey {
  uint32_t k0, k1;
  explicit PhiloxKey(uint64_t seed)
      : k0((uint32_t)(seed & 0xffffffffu)), k1((uint32_t)(seed >> 32)) {}
};
#define MIA_CHECK_COUNTER(image0, N) \
  MIA_CHECK_ARG((uint64_t)(image0) + (uint64_t)(N) <= (1ULL << 32), "image0 + N must be <= 2^32")

// The shape checks of the launchers that read the pooled gradients per image element
// (image_grad / pgd_update / grad_assemble / grad_assemble_norms): the kernels index g_vgg as
// [n][y / pf][x / pf][c < 3] of cpad channels and g_enc as
// [n][c][y / (S / enc_res)][x / (S / enc_res)].
#define MIA_CHECK_PIXEL_GRAD(N, S, pf, cpad, g_vgg, g_enc, enc_res, dtype)                      \
  MIA_CHECK_ARG((S) > 0 && (S) <= 16384, "S must be in 1 … 16384");                             \
  MIA_CHECK_ARG((N) > 0 && (N) <= 65535, "N must be in 1 … 65535");                             \
  MIA_CHECK_ARG((pf) >= 1 && (S) % (pf) == 0, "pf must divide S");                              \
  MIA_CHECK_ARG(!(g_vgg) || (cpad) >= 3, "cpad must be >= 3");                                  \
  MIA_CHECK_ARG(!(g_enc) || ((enc_res) >= 1 && (S) % (enc_res) == 0), "enc_res must divide S"); \
  MIA_CHECK_ARG((dtype) == MIA_F32 || (dtype) == MIA_F16 || (dtype) == MIA_BF16,                \
                "unsupported dtype")

extern "C" int mia_image_grad(const float* rec, const float* t, const void* g_vgg, float* g_img,
                              int N, int S, int pf, int cpad, float coef, int dtype, void* stream) {
  MIA_CHECK_ARG(rec && t && g_img, "null rec / t / g_img");
  MIA_CHECK_PIXEL_GRAD(N, S, pf, cpad, g_vgg, (const float*)nullptr, S, dtype);
  const int64_t total = (int64_t)N * 3 * S * S;
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(image_grad_kernel<T>, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, rec, t,
                 (const T*)g_vgg, g_img, N, S, pf, cpad, coef));
  return MIA_OK;
}

extern "C" int mia_pgd_update(float* x, const float* x0, const void* g_vgg, const float* g_enc,
                              int N, int S, int pf, int cpad, int enc_res, float coef_img, float a,
                              float e, float lo, float hi, int* nonfinite, int dtype,
                              void* stream) {
  MIA_CHECK_ARG(x && x0, "null x / x0");
  MIA_CHECK_ARG(lo <= hi, "need lo <= hi");
  MIA_CHECK_PIXEL_GRAD(N, S, pf, cpad, g_vgg, g_enc, enc_res, dtype);
  if (!g_enc) enc_res = S;  // unused, but the kernel divides by S / enc_res
  const int64_t total = (int64_t)N * 3 * S * S;
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(pgd_update_kernel<T>, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, x, x0,
                 (const T*)g_vgg, g_enc, N, S, pf, cpad, enc_res, coef_img, a, e, lo, hi,
                 nonfinite));
  return MIA_OK;
}

extern "C" int mia_grad_assemble(const float* x, const float* x0, const void* g_vgg,
                                 const float* g_enc, float* g, int N, int S, int pf, int cpad,
                                 int enc_res, float coef_img, float scale, int* nonfinite,
                                 int dtype, void* stream) {
  MIA_CHECK_ARG(x && x0 && g, "null x / x0 / g");
  MIA_CHECK_PIXEL_GRAD(N, S, pf, cpad, g_vgg, g_enc, enc_res, dtype);
  if (!g_enc) enc_res = S;  // unused, but the kernel divides by S / enc_res
  const int64_t total = (int64_t)N * 3 * S * S;
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(grad_assemble_kernel<T>, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, x,
                 x0, (const T*)g_vgg, g_enc, g, N, S, pf, cpad, enc_res, coef_img, scale,
                 nonfinite));
  return MIA_OK;
}

extern "C" int mia_grad_assemble_norms(const float* x, const float* x0, const void* g_vgg,
                                       const float* g_enc, float* g, float* l1, float* l2sq,
                                       int N, int S, int pf, int cpad, int enc_res,
                                       float coef_img, float scale, int* nonfinite, int dtype,
                                       void* stream) {
  MIA_CHECK_ARG(x && x0 && g, "null x / x0 / g");
  // (the plane 3·S² is below 2^31 for every S these admit: MIA_CHECK_IMAGES has nothing to add)
  MIA_CHECK_PIXEL_GRAD(N, S, pf, cpad, g_vgg, g_enc, enc_res, dtype);
  if (!g_enc) enc_res = S;  // unused, but the kernel divides by S / enc_res
  const int64_t plane = (int64_t)3 * S * S;
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(plane, {x, x0, g});
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  MIA_DISPATCH_DTYPE(dtype, T, return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("grad_assemble_norms_kernel", grad_assemble_norms_kernel<T, 4>,
                   grad_assemble_norms_kernel<T, 1>, vec, grid, 0, st, x, x0, (const T*)g_vgg,
                   g_enc, g, part, plane, S, pf, cpad, enc_res, coef_img, scale, nonfinite);
  }));
  return MIA_OK;
}

extern "C" int mia_l2_step(float* x, const float* x0, const float* g, const float* gnorm2sq,
                           float* dsq_out, int N, int64_t plane, float a, int* nonfinite,
                           void* stream) {
  MIA_CHECK_ARG(x && x0 && g && gnorm2sq && dsq_out, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(a > 0.f, "the step a must be > 0");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(plane, {x, x0, g});
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  return launch_norms(dsq_out, nullptr, grid, N, st, [&](float* part) {
    return launch2("l2_step_kernel", l2_step_kernel<4>, l2_step_kernel<1>, vec, grid, 0, st, x, x0,
                   g, gnorm2sq, part, plane, a, nonfinite);
  });
}

extern "C" int mia_l2_project(float* x, const float* x0, const float* dsq, int N, int64_t plane,
                              float e, float lo, float hi, void* stream) {
  MIA_CHECK_ARG(x && x0 && dsq, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(e > 0.f && lo <= hi, "need e > 0 and lo <= hi");
  const bool vec = vec_ok(plane, {x, x0});
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  return launch2("l2_project_kernel", l2_project_kernel<4>, l2_project_kernel<1>, vec, grid, 0,
                 (hipStream_t)stream, x, x0, dsq, plane, e, lo, hi);
}

extern "C" int mia_mi_update(float* x, const float* x0, const float* g, const float* l1, float* m,
                             int N, int64_t plane, float mu, float a, float e, float lo, float hi,
                             int* nonfinite, void* stream) {
  MIA_CHECK_ARG(x && x0 && g && l1 && m, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(mu >= 0.f && a > 0.f && e > 0.f && lo <= hi,
                "need mu >= 0, a > 0, e > 0 and lo <= hi");
  const bool vec = vec_ok(plane, {x, x0, g, m});
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  return launch2("mi_update_kernel", mi_update_kernel<4>, mi_update_kernel<1>, vec, grid, 0,
                 (hipStream_t)stream, x, x0, g, l1, m, plane, mu, a, e, lo, hi, nonfinite);
}

extern "C" int mia_ti_smooth_norms(const float* g, float* gs, const float* taps, int K, float* l1,
                                   float* l2sq, int N, int C, int H, int W, int* nonfinite,
                                   void* stream) {
  MIA_CHECK_ARG(g && gs && taps, "null g / gs / taps");
  MIA_CHECK_ARG(g != gs, "g and gs must be distinct buffers");
  MIA_CHECK_ARG(K >= 1 && K <= TI_MAXK && (K & 1), "K must be odd, in 1 … 63");
  MIA_CHECK_ARG(C > 0 && H > 0 && W > 0, "C, H and W must be > 0");
  const int64_t hw = (int64_t)H * W;  // < 2^62
  MIA_CHECK_ARG(hw < (1LL << 31), "C·H·W must be below 2^31");
  const int64_t plane = (int64_t)C * hw;
  MIA_CHECK_IMAGES(N, plane);
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(W, {g, gs});
  const int tiles_x = (W + TI_T - 1) / TI_T, tiles_y = (H + TI_T - 1) / TI_T;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
  const void* fn = vec ? (const void*)ti_smooth_norms_kernel<4>
                       : (const void*)ti_smooth_norms_kernel<1>;
  if (const int rc = ensure_dyn_lds(fn, TiGeom(TI_MAXK).floats * 4); rc != MIA_OK) return rc;
  return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("ti_smooth_norms_kernel", ti_smooth_norms_kernel<4>, ti_smooth_norms_kernel<1>,
                   vec, grid, TiGeom(K).floats * 4, st, g, gs, taps, K, part, C, H, W, tiles_x,
                   tiles_y, nonfinite);
  });
}

// the checks shared by the two input-diversity entry points; a and b: N·C·S² floats each
#define MIA_CHECK_DI(a, b, N, C, S, rnd, top, left)                                           \
  MIA_CHECK_ARG((a) && (b), "null buffer");                                                   \
  MIA_CHECK_ARG((C) > 0 && (S) > 0, "C and S must be > 0");                                   \
  MIA_CHECK_ARG((int64_t)(S) * (S) < (1LL << 31), "C·S² must be below 2^31");                 \
  MIA_CHECK_IMAGES(N, (int64_t)(C) * (S) * (S));                                              \
  MIA_CHECK_ARG((rnd) >= 1 && (rnd) <= (S), "rnd must be in 1 … S");                          \
  MIA_CHECK_ARG((top) >= 0 && (top) <= (S) - (rnd) && (left) >= 0 && (left) <= (S) - (rnd),   \
                "need top, left >= 0, top + rnd <= S and left + rnd <= S");                   \
  MIA_CHECK_ARG(disjoint({words(a, (int64_t)(N) * (C) * (S) * (S)),                           \
                          words(b, (int64_t)(N) * (C) * (S) * (S))}),                         \
                "the input and the output must be distinct buffers")

extern "C" int mia_di_resize_pad(const float* x, float* y, int N, int C, int S, int rnd, int top,
                                 int left, void* stream) {
  MIA_CHECK_DI(x, y, N, C, S, rnd, top, left);
  const bool vec = vec_ok(S, {x, y});
  const int tiles_x = (S + DI_TX - 1) / DI_TX, tiles_y = (S + DI_TY - 1) / DI_TY;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
  return launch2("di_resize_pad_kernel", di_resize_pad_kernel<true>, di_resize_pad_kernel<false>,
                 vec, grid, 0, (hipStream_t)stream, x, y, C, S, rnd, top, left, tiles_x, tiles_y);
}

extern "C" int mia_di_resize_pad_bwd_norms(const float* g, float* gx, float* l1, float* l2sq,
                                           int N, int C, int S, int rnd, int top, int left,
                                           int* nonfinite, void* stream) {
  MIA_CHECK_DI(g, gx, N, C, S, rnd, top, left);
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(S, {g, gx});
  const int tiles_x = (S + DI_TX - 1) / DI_TX, tiles_y = (S + DI_TY - 1) / DI_TY;
  const dim3 grid(C * tiles_x * tiles_y, N);
  return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("di_resize_pad_bwd_norms_kernel", di_resize_pad_bwd_norms_kernel<true>,
                   di_resize_pad_bwd_norms_kernel<false>, vec, grid, 0, st, g, gx, part, C, S, rnd,
                   top, left, tiles_x, tiles_y, nonfinite);
  });
}

// s = 2^-i for 0 ≤ i < MIA_SI_MAX_SCALES (NaN fails every comparison)
static inline bool si_scale_ok(float s) {
  for (int i = 0; i < MIA_SI_MAX_SCALES; ++i)
    if (s == ldexpf(1.f, -i)) return true;
  return false;
}

extern "C" int mia_si_transform(const float* x, const float* m, float* y, int N, int64_t plane,
                                float c, float s, void* stream) {
  MIA_CHECK_ARG(x && y, "null x / y");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(si_scale_ok(s), "s must be 2^-i with 0 <= i < MIA_SI_MAX_SCALES");
  MIA_CHECK_ARG(__builtin_isfinite(c), "c must be finite");
  const int64_t len = (int64_t)N * plane;
  const Span Y = words(y, len);
  MIA_CHECK_ARG(disjoint({words(x, len), Y}) && disjoint({words(m, len), Y}),
                "the inputs and the output must be distinct buffers");
  const bool vec = vec_ok(plane, {x, y, m});
  const dim3 grid = image_grid(plane + 3, 4, N);
  return launch2("si_transform_kernel", si_transform_kernel<true>, si_transform_kernel<false>, vec,
                 grid, 0, (hipStream_t)stream, x, m, y, plane, c, s);
}

extern "C" int mia_si_accumulate_norms(const float* g, float* acc, float* l1, float* l2sq, int N,
                                       int64_t plane, float w, int first, float div,
                                       int* nonfinite, void* stream) {
  MIA_CHECK_ARG(g && acc, "null g / acc");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(si_scale_ok(w), "w must be 2^-i with 0 <= i < MIA_SI_MAX_SCALES");
  MIA_CHECK_ARG(__builtin_isfinite(div) && div >= 1.f, "div must be finite and >= 1");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(disjoint({words(g, len), words(acc, len)}), "g and acc must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(plane, {g, acc});
  const dim3 grid = image_grid(plane + 3, 4, N);
  return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("si_accumulate_norms_kernel", si_accumulate_norms_kernel<true>,
                   si_accumulate_norms_kernel<false>, vec, grid, 0, st, g, acc, part, plane, w,
                   first != 0, div, nonfinite);
  });
}

extern "C" int mia_vt_neighbor(const float* x, const float* m, float* y, int N, int64_t plane,
                               float c, float r, uint64_t seed, uint32_t image0, uint32_t step,
                               uint32_t sample, void* stream) {
  MIA_CHECK_ARG(x && y, "null x / y");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_COUNTER(image0, N);
  MIA_CHECK_ARG(__builtin_isfinite(c), "c must be finite");
  MIA_CHECK_ARG(__builtin_isfinite(r) && r >= 0.f, "r must be finite and >= 0");
  const int64_t len = (int64_t)N * plane;
  const Span Y = words(y, len);
  MIA_CHECK_ARG(disjoint({words(x, len), Y}) && disjoint({words(m, len), Y}),
                "the inputs and the output must be distinct buffers");
  const bool vec = vec_ok(plane, {x, y, m});
  const dim3 grid = image_grid(plane + 3, 4, N);
  const PhiloxKey key(seed);
  return launch2("vt_neighbor_kernel", vt_neighbor_kernel<true>, vt_neighbor_kernel<false>, vec,
                 grid, 0, (hipStream_t)stream, x, m, y, plane, c, r, key.k0, key.k1, image0, step,
                 sample);
}

extern "C" int mia_vt_combine_norms(const float* g, const float* gv, float* v, float* gt,
                                    float* l1, int N, int64_t plane, int* nonfinite,
                                    void* stream) {
  MIA_CHECK_ARG(g && v && gt, "null g / v / gt");
  MIA_CHECK_IMAGES(N, plane);
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(disjoint({words(g, len), words(gv, len), words(v, len), words(gt, len)}),
                "g, gv, v and gt must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(plane, {g, gv, v, gt});
  const dim3 grid = image_grid(plane + 3, 4, N);
  return launch_norms(l1, nullptr, grid, N, st, [&](float* part) {
    return launch2("vt_combine_norms_kernel", vt_combine_norms_kernel<true>,
                   vt_combine_norms_kernel<false>, vec, grid, 0, st, g, gv, v, gt, part, plane,
                   nonfinite);
  });
}

extern "C" int mia_spsa_probe(const float* x, float* yp, float* ym, int N, int64_t plane, float d,
                              float lo, float hi, uint64_t seed, uint32_t image0, uint32_t step,
                              uint32_t sample, void* stream) {
  MIA_CHECK_ARG(x && yp && ym, "null x / yp / ym");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_COUNTER(image0, N);
  MIA_CHECK_ARG(__builtin_isfinite(d) && d > 0.f, "d must be finite and > 0");
  MIA_CHECK_ARG(lo <= hi, "need lo <= hi");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(disjoint({words(x, len), words(yp, len), words(ym, len)}),
                "x, yp and ym must be distinct buffers");
  const bool vec = vec_ok(plane, {x, yp, ym});
  const dim3 grid = image_grid(plane + 3, 4, N);
  const PhiloxKey key(seed);
  return launch2("spsa_probe_kernel", spsa_probe_kernel<true>, spsa_probe_kernel<false>, vec, grid,
                 0, (hipStream_t)stream, x, yp, ym, plane, d, lo, hi, key.k0, key.k1, image0, step,
                 sample);
}

extern "C" int mia_spsa_accumulate_norms(float* acc, const float* fp, const float* fm, float* l1,
                                         float* l2sq, int N, int64_t plane, float s, uint64_t seed,
                                         uint32_t image0, uint32_t step, uint32_t sample, int first,
                                         float div, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(acc && fp && fm, "null acc / fp / fm");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_COUNTER(image0, N);
  MIA_CHECK_ARG(__builtin_isfinite(s) && s > 0.f, "s must be finite and > 0");
  MIA_CHECK_ARG(__builtin_isfinite(div) && div > 0.f, "div must be finite and > 0");
  // acc: N·plane floats; fp, fm: N floats each
  MIA_CHECK_ARG(disjoint({words(acc, (int64_t)N * plane), words(fp, N), words(fm, N)}),
                "acc, fp and fm must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(plane, {acc});
  const dim3 grid = image_grid(plane + 3, 4, N);
  const PhiloxKey key(seed);
  return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("spsa_accumulate_norms_kernel", spsa_accumulate_norms_kernel<true>,
                   spsa_accumulate_norms_kernel<false>, vec, grid, 0, st, acc, fp, fm, part, plane,
                   s, key.k0, key.k1, image0, step, sample, first != 0, div, nonfinite);
  });
}

// Block rows of mia_uap_accumulate's grid: 1 = the loop form (a thread walks all N images and
// stores its group), > 1 = the image-split form on integer atomics. Both are exact; DESIGN.md
// records the A/B behind the default.
#ifndef MIA_UAP_SPLIT
#define MIA_UAP_SPLIT 1
#endif

extern "C" int mia_uap_accumulate(const float* g, const float* l1, int64_t* acc, int N,
                                  int64_t plane, int first, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(g && l1 && acc, "null g / l1 / acc");
  MIA_CHECK_IMAGES(N, plane);
  // |ĝ| < 2·plane (the kernel drops anything else), so |q| = |rint(ĝ·2^24)| ≤ 2^25·plane and the
  // sum over n images stays below n·plane·2^25 < 2^62 for n·plane < 2^37: no int64 overflow, with
  // a factor 2 to spare for the fp32 rounding of 2·plane. The same bound holds job-wide when the
  // caller adds the planes of several calls or ranks (attack() checks it with the job's n).
  MIA_CHECK_ARG((int64_t)N * plane < (1LL << 37), "N * plane must be < 2^37");
  MIA_CHECK_ARG(((uintptr_t)acc & 7) == 0, "acc must be 8-byte aligned");
  const Span A = {acc, plane * 8};
  MIA_CHECK_ARG(disjoint({words(g, (int64_t)N * plane), words(l1, N), A, words(nonfinite, N)}),
                "g, l1, acc and nonfinite must be distinct buffers");
  const bool vec = vec_ok(plane, {g, acc});
  const int rows = MIA_UAP_SPLIT < N ? MIA_UAP_SPLIT : N;
  const dim3 grid(blocks_for((plane + 3) / 4, TPB), rows);
  if (rows > 1 && first) {
    const int rc = mia_memset(acc, 0, A.bytes, stream);
    if (rc != MIA_OK) return rc;
  }
  return launch2("uap_accumulate_kernel", uap_accumulate_kernel<true>, uap_accumulate_kernel<false>,
                 vec, grid, 0, (hipStream_t)stream, g, l1, (long long*)acc, N, plane, first != 0,
                 nonfinite);
}

extern "C" int mia_uap_step(float* delta, const int64_t* acc, float* x, const float* x0, int N,
                            int64_t plane, float a, float e, float lo, float hi, void* stream) {
  MIA_CHECK_ARG(delta, "null delta");
  MIA_CHECK_ARG(N >= 0 && N <= 65535, "N must be in 0 … 65535");
  MIA_CHECK_ARG(plane > 0 && plane < (1LL << 31), "plane must be in 1 … 2^31 − 1");
  MIA_CHECK_ARG(N > 0 ? (x && x0) : (!x && !x0), "x and x0: both for N > 0, both NULL for N = 0");
  MIA_CHECK_ARG(N > 0 || acc, "nothing to do: N = 0 and acc = NULL");
  MIA_CHECK_ARG(a >= 0.f && e > 0.f && lo <= hi, "need a >= 0, e > 0 and lo <= hi");
  MIA_CHECK_ARG(!acc || ((uintptr_t)acc & 7) == 0, "acc must be 8-byte aligned");
  const Span D = words(delta, plane), A = {acc, plane * 8};
  MIA_CHECK_ARG(disjoint({D, A}), "delta and acc must be distinct");
  if (N > 0)
    MIA_CHECK_ARG(disjoint({words(x, (int64_t)N * plane), words(x0, (int64_t)N * plane), D, A}),
                  "delta, acc, x and x0 must be distinct buffers");
  const bool vec = vec_ok(plane, {delta, acc, x, x0});
  const dim3 grid(blocks_for((plane + 3) / 4, TPB));
  return launch2("uap_step_kernel", uap_step_kernel<true>, uap_step_kernel<false>, vec, grid, 0,
                 (hipStream_t)stream, delta, (const long long*)acc, x, x0, N, plane, a, e, lo, hi);
}

extern "C" int mia_apgd_update(float* x, float* x_old, const float* x0, const float* g,
                               const float* eta, int N, int64_t plane, float a, float e, float lo,
                               float hi, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(x && x_old && x0 && g && eta, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(a > 0.f && a <= 1.f, "the momentum weight a must be in (0, 1]");
  MIA_CHECK_ARG(e > 0.f && __builtin_isfinite(e) && lo <= hi, "need a finite e > 0 and lo <= hi");
  // the two written buffers against each other and against both inputs (x0 and g may alias)
  const int64_t len = (int64_t)N * plane;
  const Span X = words(x, len), XO = words(x_old, len);
  MIA_CHECK_ARG(disjoint({X, XO, words(x0, len)}) && disjoint({X, XO, words(g, len)}),
                "x, x_old, x0 and g must be distinct buffers");
  const bool vec = vec_ok(plane, {x, x_old, x0, g});
  const dim3 grid = image_grid(plane + 3, 4, N);
  return launch2("apgd_update_kernel", apgd_update_kernel<true>, apgd_update_kernel<false>, vec,
                 grid, 0, (hipStream_t)stream, x, x_old, x0, g, eta, plane, a, e, lo, hi,
                 nonfinite);
}

extern "C" int mia_apgd_decide(const float* loss, float* fstate, int* istate, int* action,
                               float* hist_loss, float* hist_eta, int N, int step, int checkpoint,
                               int thr, float eta0, void* stream) {
  MIA_CHECK_ARG(loss && fstate && istate && action && hist_loss && hist_eta, "null argument");
  MIA_CHECK_ARG(N > 0 && N <= 65535, "N must be in 1 … 65535");
  MIA_CHECK_ARG(step >= 0, "step must be >= 0");
  MIA_CHECK_ARG(checkpoint == 0 || checkpoint == 1, "checkpoint must be 0 or 1");
  MIA_CHECK_ARG(thr >= 0, "the threshold must be >= 0");
  MIA_CHECK_ARG(step > 0 || !checkpoint, "the start (step 0) is no checkpoint");
  MIA_CHECK_ARG(step > 0 || (eta0 > 0.f && __builtin_isfinite(eta0)),
                "the start (step 0) needs a finite eta0 > 0");
  // fstate 4·N floats, istate 3·N ints, the others N words
  MIA_CHECK_ARG(disjoint({words(loss, N), words(fstate, 4LL * N), words(istate, 3LL * N),
                          words(action, N), words(hist_loss, N), words(hist_eta, N)}),
                "the state, action, loss and history arrays must be distinct buffers");
  MIA_LAUNCH(apgd_decide_kernel, dim3((N + 63) / 64), dim3(64), 0, loss, fstate, istate, action,
             hist_loss, hist_eta, N, step, checkpoint, thr, eta0);
}

extern "C" int mia_apgd_apply(float* x, float* g, float* x_best, float* g_best, const int* action,
                              int N, int64_t plane, void* stream) {
  MIA_CHECK_ARG(x && g && x_best && g_best && action, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(disjoint({words(x, len), words(g, len), words(x_best, len), words(g_best, len)}),
                "x, g, x_best and g_best must be distinct buffers");
  const bool vec = vec_ok(plane, {x, g, x_best, g_best});
  const dim3 grid = image_grid(plane + 3, 4, N);
  return launch2("apgd_apply_kernel", apgd_apply_kernel<true>, apgd_apply_kernel<false>, vec, grid,
                 0, (hipStream_t)stream, x, g, x_best, g_best, action, plane);
}

extern "C" int mia_sh_flip(float* x, const float* x0, int8_t* s, const int* accept, int N,
                           int64_t plane, int64_t prev_lo, int64_t prev_hi, int64_t lo, int64_t hi,
                           float e, float lo_v, float hi_v, void* stream) {
  MIA_CHECK_ARG(x && x0 && s, "null x / x0 / s");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(0 <= prev_lo && prev_lo <= prev_hi && prev_hi <= plane,
                "need 0 <= prev_lo <= prev_hi <= plane");
  MIA_CHECK_ARG(0 <= lo && lo <= hi && hi <= plane, "need 0 <= lo <= hi <= plane");
  MIA_CHECK_ARG(prev_lo < prev_hi || lo < hi, "both ranges are empty: nothing to do");
  MIA_CHECK_ARG(__builtin_isfinite(e) && e > 0.f, "e must be finite and > 0");
  MIA_CHECK_ARG(lo_v <= hi_v, "need lo_v <= hi_v");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(disjoint({words(x, len), words(x0, len), Span{s, len}, words(accept, N)}),
                "x, x0, s and accept must be distinct buffers");
  // the hull of the non-empty ranges, in groups of 4 elements counted from the image start
  const bool hp = prev_lo < prev_hi, hn = lo < hi;
  const int64_t h0 = hp && hn ? (prev_lo < lo ? prev_lo : lo) : hp ? prev_lo : lo;
  const int64_t h1 = hp && hn ? (prev_hi > hi ? prev_hi : hi) : hp ? prev_hi : hi;
  const int64_t g0 = h0 / 4, ng = (h1 + 3) / 4 - g0;
  const bool vec = vec_ok(plane, {x, x0}) && ((uintptr_t)s & 3) == 0;
  const dim3 grid(blocks_for(ng, TPB, 1024), N);
  return launch2("sh_flip_kernel", sh_flip_kernel<true>, sh_flip_kernel<false>, vec, grid, 0,
                 (hipStream_t)stream, x, x0, (signed char*)s, accept, plane, g0, ng, prev_lo,
                 prev_hi, lo, hi, e, lo_v, hi_v);
}

extern "C" int mia_sh_decide(const float* loss, float* best, int* accept, int* n_accept,
                             float* hist_loss, int N, int first, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(loss && best && accept && n_accept && hist_loss, "null argument");
  MIA_CHECK_ARG(N > 0 && N <= 65535, "N must be in 1 … 65535");
  MIA_CHECK_ARG(first == 0 || first == 1, "first must be 0 or 1");
  MIA_CHECK_ARG(disjoint({words(loss, N), words(best, N), words(accept, N), words(n_accept, N),
                          words(hist_loss, N), words(nonfinite, N)}),
                "loss, best, accept, n_accept, hist_loss and nonfinite must be distinct buffers");
  MIA_LAUNCH(sh_decide_kernel, dim3((N + 63) / 64), dim3(64), 0, loss, best, accept, n_accept,
             hist_loss, N, first, nonfinite);
}

extern "C" int mia_pi_update(float* x, const float* x0, const float* g, const float* l1,
                             const float* m_in, float* m_out, const float* A_in, float* A_out,
                             int N, int C, int H, int W, int K, float mu, float ab, float gm,
                             float e, float lo, float hi, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(x && x0 && g && l1 && m_in && m_out && A_in && A_out, "null argument");
  MIA_CHECK_ARG(K >= 3 && K <= PI_MAXK && (K & 1), "K must be odd, in 3 … 15");
  MIA_CHECK_ARG(C > 0 && H > 0 && W > 0, "C, H and W must be > 0");
  const int64_t hw = (int64_t)H * W;  // < 2^62
  MIA_CHECK_ARG(hw < (1LL << 31), "C·H·W must be below 2^31");
  const int64_t plane = (int64_t)C * hw;
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(__builtin_isfinite(mu) && mu >= 0.f, "mu must be finite and >= 0");
  MIA_CHECK_ARG(__builtin_isfinite(ab) && ab >= 0.f && __builtin_isfinite(gm) && gm >= 0.f &&
                    __builtin_isfinite(e) && e >= 0.f,
                "ab, gm and e must be finite and >= 0");
  MIA_CHECK_ARG(lo <= hi, "need lo <= hi");
  // m and A ping-pong (a block's halo reads what its neighbours would overwrite); no written
  // buffer may overlap any other, while the inputs may alias each other
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!overlap(words(m_in, len), words(m_out, len)),
                "m_in and m_out must be distinct buffers");
  MIA_CHECK_ARG(!overlap(words(A_in, len), words(A_out, len)),
                "A_in and A_out must be distinct buffers");
  const float* wr[3] = {x, m_out, A_out};
  const float* rd[7] = {x0, g, m_in, A_in, x, m_out, A_out};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 7; ++j)
      MIA_CHECK_ARG(j == i + 4 || !overlap(words(wr[i], len), words(rd[j], len)),
                    "x, x0, g, m_in, m_out, A_in and A_out must be distinct buffers");
  for (int i = 0; i < 3; ++i)
    MIA_CHECK_ARG(!overlap(words(l1, N), words(wr[i], len)),
                  "l1 must not overlap x, m_out or A_out");
  const bool vec = vec_ok(W, {x, x0, g, m_in, m_out, A_in, A_out});
  const int tiles_x = (W + TI_T - 1) / TI_T, tiles_y = (H + TI_T - 1) / TI_T;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
#define MIA_PI_CASE(k)                                                                           \
  case k:                                                                                        \
    return launch2("pi_update_kernel", pi_update_kernel<k, true>, pi_update_kernel<k, false>, vec, \
                   grid, 0, (hipStream_t)stream, x, x0, g, l1, m_in, m_out, A_in, A_out, C, H, W, \
                   tiles_x, tiles_y, mu, ab, gm, e, lo, hi, nonfinite)
  switch (K) {
    MIA_PI_CASE(3);
    MIA_PI_CASE(5);
    MIA_PI_CASE(7);
    MIA_PI_CASE(9);
    MIA_PI_CASE(11);
    MIA_PI_CASE(13);
    MIA_PI_CASE(15);
  }
#undef MIA_PI_CASE
  return set_error("mia_pi_update: unsupported K");
}

extern "C" int mia_cw_init(const float* x, float* w, int64_t len, void* stream) {
  MIA_CHECK_ARG(x && w && len > 0, "bad args");
  MIA_LAUNCH(cw_init_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, x, w, len);
}

extern "C" int mia_cw_tanh(const float* w, float* adv, int64_t len, void* stream) {
  MIA_CHECK_ARG(w && adv && len > 0, "bad args");
  MIA_LAUNCH(cw_tanh_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, w, adv, len);
}

extern "C" int mia_cw_grad(const float* adv, const float* x, const float* g_f, float* g_w,
                           int64_t len, float c, float scale, void* stream) {
  MIA_CHECK_ARG(adv && x && g_f && g_w && len > 0, "bad args");
  MIA_LAUNCH(cw_grad_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, adv, x, g_f, g_w,
             len, c, scale);
}

extern "C" int mia_cw_select(const float* adv, float* best_adv, const float* sq, float* best_l2,
                             const float* f, const float* f0, int N, int64_t plane, float l2_scale,
                             void* stream) {
  MIA_CHECK_ARG(adv && best_adv && sq && best_l2 && f && f0 && N > 0 && plane > 0, "bad args");
  MIA_LAUNCH(cw_select_kernel, dim3(N), dim3(TPB), 0, adv, best_adv, sq, best_l2, f, f0, plane,
             l2_scale);
}

extern "C" int mia_random_start(float* x, const float* x0, const float* u, int64_t len, float e,
                                float lo, float hi, void* stream) {
  MIA_CHECK_ARG(x && x0 && u && len > 0, "bad args");
  MIA_LAUNCH(random_start_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, x, x0, u, len,
             e, lo, hi);
}

extern "C" int mia_sign_project(float* x, const float* x0, const float* g, int64_t len, float a,
                                float e, float lo, float hi, void* stream) {
  MIA_CHECK_ARG(x && x0 && g && len > 0, "bad args");
  MIA_LAUNCH(sign_project_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, x, x0, g, len,
             a, e, lo, hi);
}

extern "C" int mia_adam_step(float* p, const float* g, float* m, float* v, int64_t len, float lr,
                             float beta1, float beta2, float eps, int t, void* stream) {
  MIA_CHECK_ARG(p && g && m && v && len > 0 && t >= 1, "bad args");
  const float bc1 = 1.f - powf(beta1, (float)t);
  const float bc2sqrt = sqrtf(1.f - powf(beta2, (float)t));
  MIA_LAUNCH(adam_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, p, g, m, v, len, lr,
             beta1, beta2, eps, bc1, bc2sqrt);
}

extern "C" int mia_patch_update(float* patch, const float* g, const float* img, const float* mask,
                                float* adv, int64_t len, int64_t shared, float lo, float hi,
                                void* stream) {
  MIA_CHECK_ARG(patch && img && mask && adv && len > 0 && shared >= 0 && lo <= hi, "bad args");
  MIA_CHECK_ARG(!g || !shared, "a gradient step needs a per-image patch (shared = 0)");
  MIA_CHECK_ARG(!shared || len % shared == 0, "len must be a multiple of shared");
  MIA_LAUNCH(patch_update_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, patch, g, img,
             mask, adv, len, shared, lo, hi);
}
