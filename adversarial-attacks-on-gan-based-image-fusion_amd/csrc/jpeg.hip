// JPEG round trip (baseline, 4:4:4) and the adjoint of its differentiable surrogate (gfx950): what
// saving an adversarial image as .jpg and loading it again does to it, as one more stage of the
// attack's step-gradient chain (pgd.AttackEngine._step_gradient). Images are fp32 NCHW planes in
// [-1,1], S % 8 == 0. The arithmetic and its order are in include/miattack.h; every operation is
// one fp32 rounding with no contraction, so the torch fp32 reference (tests/jpeg_ref.py)
// reproduces the bits.
//
// One block of TPB = 256 threads owns a tile of 64 × 32 pixels = 8 × 4 blocks of 8 × 8, of all
// three planes of one image (the colour conversion needs the three channels of a pixel). The tile
// lives in LDS as [plane][32 rows][JP_LD = 68 floats] and is transformed in place:
//   * load / store passes: a thread moves 16-byte vectors, 16 lanes per tile row (256 contiguous
//     bytes of global memory); 8 consecutive lanes write 32 consecutive LDS dwords;
//   * row passes: thread (row = t % 32, block column = t / 32) owns 8 consecutive floats, two
//     ds_read_b128 / ds_write_b128. The stride 68 puts row r's 16-byte slot at (r + const) mod 16
//     of the 256-byte bank row, and every 16-lane group of a b128 read holds rows that are
//     distinct mod 16 (0–3, 12–15, 20–27 and 4–11, 16–19, 28–31). The in-place ds_write_b128 is
//     served 8 contiguous lanes at a time on 32 banks: rows r … r + 7 start at dword 4·r mod 32
//     and cover 4 banks each, all 32 once. Unpadded (stride 64) all 32 rows of a half wave would
//     sit on one slot;
//   * column passes: thread (column = t % 64, block row = t / 64) owns 8 floats one tile row
//     apart; the 64 lanes of a wave read and write 64 consecutive dwords per row;
//   * the store pass reads rows back 16 lanes per row; with the padded stride one 16-lane group
//     of its ds_read_b128 spans two rows and two of its lanes share a slot (2-way on 1 of 16).
// These conflict counts are DERIVED from the bank rule; what was measured is in DESIGN.md §8.
// Where S is no multiple of the tile, the positions beyond the image hold zeros and are never
// stored; S % 8 == 0 keeps every 8 × 8 block whole.
#include "attack_common.h"

namespace mia {

constexpr int JP_TX = 64, JP_TY = 32;
constexpr int JP_LD = JP_TX + 4;
constexpr int JP_PLANE = JP_TY * JP_LD;

// D[u][i] = c(u)/2·cos((2i+1)·u·π/16), c(0) = 1/√2: evaluated in fp64 and rounded once to fp32
// (pgd.jpeg_dct_matrix() returns the same bits). cos(k·π/16)/2 for k = 1 … 7, and 1/(2√2) = C4.
#define JC1 0x1.f6297cp-2f
#define JC2 0x1.d906bcp-2f
#define JC3 0x1.a9b662p-2f
#define JC4 0x1.6a09e6p-2f
#define JC5 0x1.1c73b4p-2f
#define JC6 0x1.87de2ap-3f
#define JC7 0x1.8f8b84p-4f
static __constant__ const float JD[8][8] = {
    {JC4, JC4, JC4, JC4, JC4, JC4, JC4, JC4},
    {JC1, JC3, JC5, JC7, -JC7, -JC5, -JC3, -JC1},
    {JC2, JC6, -JC6, -JC2, -JC2, -JC6, JC6, JC2},
    {JC3, -JC7, -JC1, -JC5, JC5, JC1, JC7, -JC3},
    {JC4, -JC4, -JC4, JC4, JC4, -JC4, -JC4, JC4},
    {JC5, -JC1, JC7, JC3, -JC3, -JC7, JC1, -JC5},
    {JC6, -JC2, JC2, -JC6, -JC6, JC2, -JC2, JC6},
    {JC7, -JC5, JC3, -JC1, JC1, -JC3, JC5, -JC7}};

// o[u] = Σ_k D[u][k]·v[k] (the DCT-II along one axis) or, INV, o[i] = Σ_k D[k][i]·v[k] (its
// inverse, D is orthonormal): d[0]·v[0], then + d[k]·v[k] for k = 1 … 7, a mul, then a mul and an
// add per term.
template <bool INV>
__device__ __forceinline__ void dct8(const float (&v)[8], float (&o)[8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    float s = (INV ? JD[0][u] : JD[u][0]) * v[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float p = (INV ? JD[k][u] : JD[u][k]) * v[k];
      s = s + p;
    }
    o[u] = s;
  }
}

// 4 consecutive floats of a plane row: one 16-byte access (VEC) or 4 scalars, the same bits
template <bool VEC>
__device__ __forceinline__ void ld4(const float* __restrict__ p, float (&v)[4]) {
  if (VEC) {
    ldv<4>(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p[e];
  }
}

template <bool VEC>
__device__ __forceinline__ void st4(float* __restrict__ p, const float (&v)[4]) {
  if (VEC) {
    stv<4>(p, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = v[e];
  }
}

// The load / store passes' position q ∈ {0, 1} of thread t: tile row, tile column (a multiple of
// 4) and whether the 4 pixels lie inside the image (S % 4 == 0: all or none).
struct JpPos {
  int row, col;
  bool in;
  int64_t off;  // within a plane
};
__device__ __forceinline__ JpPos jp_pos(int t, int q, int ty0, int tx0, int S) {
  const int pos = t + q * TPB;
  JpPos p;
  p.row = pos >> 4;
  p.col = (pos & 15) * 4;
  p.in = ty0 + p.row < S && tx0 + p.col < S;
  p.off = (int64_t)(ty0 + p.row) * S + (tx0 + p.col);
  return p;
}

// steps 1 and 2: the 8-bit pixel p = floor(clamp((x + 1)·127.5 + 0.5, 0, 255)) of the three
// channels and the JFIF RGB → YCbCr (products added left to right; Y − 128, the ±128 of Cb and
// Cr cancels) into the LDS tile
template <bool VEC>
__device__ __forceinline__ void jp_load_ycc(const float* __restrict__ xp, int64_t hw, int S,
                                            int ty0, int tx0, float* __restrict__ sm) {
#pragma clang fp contract(off)
  for (int q = 0; q < 2; ++q) {
    const JpPos p = jp_pos(threadIdx.x, q, ty0, tx0, S);
    float c[3][4], o[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int e = 0; e < 4; ++e) c[ch][e] = 0.f;
      if (p.in) ld4<VEC>(xp + ch * hw + p.off, c[ch]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float px[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float a = c[ch][e] + 1.f;
        const float b = a * 127.5f;
        const float d = b + 0.5f;
        px[ch] = floorf(fminf(fmaxf(d, 0.f), 255.f));
      }
      const float y0 = 0.299f * px[0], y1 = 0.587f * px[1], y2 = 0.114f * px[2];
      const float b0 = -0.168736f * px[0], b1 = -0.331264f * px[1], b2 = 0.5f * px[2];
      const float r0 = 0.5f * px[0], r1 = -0.418688f * px[1], r2 = -0.081312f * px[2];
      const float ys = (y0 + y1) + y2;
      o[0][e] = p.in ? ys - 128.f : 0.f;
      o[1][e] = p.in ? (b0 + b1) + b2 : 0.f;
      o[2][e] = p.in ? (r0 + r1) + r2 : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) stv<4>(sm + ch * JP_PLANE + p.row * JP_LD + p.col, o[ch]);
  }
}

// 8 consecutive floats of an LDS tile row, as two 16-byte accesses
__device__ __forceinline__ void lds_ld8(const float* __restrict__ p, float (&v)[8]) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}

__device__ __forceinline__ void lds_st8(float* __restrict__ p, const float (&v)[8]) {
  f32x4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = v[e];
    b[e] = v[4 + e];
  }
  *(f32x4*)p = a;
  *(f32x4*)(p + 4) = b;
}

// the forward row pass of the three planes, in place
__device__ __forceinline__ void jp_rows_fwd(float* __restrict__ sm) {
  const int row = threadIdx.x & 31, bc = threadIdx.x >> 5;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* __restrict__ p = sm + ch * JP_PLANE + row * JP_LD + bc * 8;
    float v[8], o[8];
    lds_ld8(p, v);
    dct8<false>(v, o);
    lds_st8(p, o);
  }
}

// the inverse row pass of the three planes into registers: o[ch][0 … 7] of this thread's row
__device__ __forceinline__ void jp_rows_inv(const float* __restrict__ sm, float (&o)[3][8]) {
  const int row = threadIdx.x & 31, bc = threadIdx.x >> 5;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* __restrict__ p = sm + ch * JP_PLANE + row * JP_LD + bc * 8;
    float v[8];
    lds_ld8(p, v);
    dct8<true>(v, o[ch]);
  }
}

__device__ __forceinline__ void jp_rows_put(float* __restrict__ sm, const float (&o)[3][8]) {
  const int row = threadIdx.x & 31, bc = threadIdx.x >> 5;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* __restrict__ p = sm + ch * JP_PLANE + row * JP_LD + bc * 8;
    lds_st8(p, o[ch]);
  }
}

// This thread's column of plane ch (column = t % 64, block row = t / 64), 8 floats one row apart
__device__ __forceinline__ float* jp_col(float* __restrict__ sm, int ch) {
  return sm + ch * JP_PLANE + (threadIdx.x >> 6) * 8 * JP_LD + (threadIdx.x & 63);
}

// the quantiser steps of this thread's column: Q[ch ? 1 : 0][k·8 + column % 8], k = the vertical
// frequency
__device__ __forceinline__ void jp_qcol(const float* __restrict__ qtab, float (&q)[2][8]) {
#pragma unroll
  for (int tb = 0; tb < 2; ++tb)
#pragma unroll
    for (int k = 0; k < 8; ++k) q[tb][k] = qtab[tb * 64 + k * 8 + (threadIdx.x & 7)];
}

// y = J(x), the five steps of the header.
template <bool VEC>
__global__ __launch_bounds__(TPB) void jpeg_roundtrip_kernel(const float* __restrict__ x,
                                                             float* __restrict__ y,
                                                             const float* __restrict__ qtab, int S,
                                                             int tiles_x) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sm[3 * JP_PLANE];
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * JP_TY, tx0 = (blockIdx.x % tiles_x) * JP_TX;
  const int64_t hw = (int64_t)S * S;
  const float* __restrict__ xp = x + (int64_t)n * 3 * hw;
  float* __restrict__ yp = y + (int64_t)n * 3 * hw;
  float q[2][8];
  jp_qcol(qtab, q);
  jp_load_ycc<VEC>(xp, hw, S, ty0, tx0, sm);
  __syncthreads();
  jp_rows_fwd(sm);
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* __restrict__ p = jp_col(sm, ch);
    float v[8], f[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[k * JP_LD];
    dct8<false>(v, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float qq = q[ch ? 1 : 0][k];
      const float vv = f[k] / qq;
      f[k] = rintf(vv) * qq;
    }
    dct8<true>(f, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * JP_LD] = o[k];
  }
  __syncthreads();
  {
    float o[3][8];
    jp_rows_inv(sm, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float yv = o[0][e] + 128.f, cb = o[1][e], cr = o[2][e];
      const float r1 = 1.402f * cr;
      const float g1 = -0.344136f * cb, g2 = -0.714136f * cr;
      const float b1 = 1.772f * cb;
      const float rgb[3] = {yv + r1, (yv + g1) + g2, yv + b1};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float pq = fminf(fmaxf(rintf(rgb[ch]), 0.f), 255.f);
        const float d = pq / 127.5f;
        o[ch][e] = d - 1.f;
      }
    }
    jp_rows_put(sm, o);
  }
  __syncthreads();
  for (int qi = 0; qi < 2; ++qi) {
    const JpPos p = jp_pos(threadIdx.x, qi, ty0, tx0, S);
    if (!p.in) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[4];
      ldv<4>(sm + ch * JP_PLANE + p.row * JP_LD + p.col, v);
      st4<VEC>(yp + ch * hw + p.off, v);
    }
  }
}

// gx = Aᵀ·IDCT(w ⊙ DCT(Mᵀ·g)), w = 3·(v − rint(v))² at the coefficients v of x: the adjoint of
// the round trip whose coefficient rounding is replaced by Shin & Song's round(v) + (v − round(v))³
// (the pixel roundings and clamps pass the gradient through; the 127.5 factors and Q cancel). The
// launch recomputes v from x (steps 1 – 4), keeps w in 24 registers per thread — the two column
// passes map threads to coefficients alike — and reuses the one LDS tile for g.
template <bool VEC>
__global__ __launch_bounds__(TPB) void jpeg_bwd_norms_kernel(
    const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gx,
    const float* __restrict__ qtab, float* __restrict__ part, int S, int tiles_x,
    int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sm[3 * JP_PLANE];
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * JP_TY, tx0 = (blockIdx.x % tiles_x) * JP_TX;
  const int64_t hw = (int64_t)S * S;
  const float* __restrict__ xp = x + (int64_t)n * 3 * hw;
  const float* __restrict__ gp = g + (int64_t)n * 3 * hw;
  float* __restrict__ op = gx + (int64_t)n * 3 * hw;
  float w[3][8];
  {
    float q[2][8];
    jp_qcol(qtab, q);
    jp_load_ycc<VEC>(xp, hw, S, ty0, tx0, sm);
    __syncthreads();
    jp_rows_fwd(sm);
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* __restrict__ p = jp_col(sm, ch);
      float v[8], f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = p[k * JP_LD];
      dct8<false>(v, f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float vv = f[k] / q[ch ? 1 : 0][k];
        const float d = vv - rintf(vv);
        const float dd = d * d;
        w[ch][k] = 3.f * dd;
      }
    }
    __syncthreads();
  }
  // h = Mᵀ·g: (Y, Cb, Cr) components of the RGB gradient
  for (int qi = 0; qi < 2; ++qi) {
    const JpPos p = jp_pos(threadIdx.x, qi, ty0, tx0, S);
    float c[3][4], o[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int e = 0; e < 4; ++e) c[ch][e] = 0.f;
      if (p.in) ld4<VEC>(gp + ch * hw + p.off, c[ch]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = c[0][e], gg = c[1][e], gb = c[2][e];
      const float b0 = -0.344136f * gg, b1 = 1.772f * gb;
      const float r0 = 1.402f * gr, r1 = -0.714136f * gg;
      o[0][e] = (gr + gg) + gb;
      o[1][e] = b0 + b1;
      o[2][e] = r0 + r1;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) stv<4>(sm + ch * JP_PLANE + p.row * JP_LD + p.col, o[ch]);
  }
  __syncthreads();
  jp_rows_fwd(sm);
  __syncthreads();
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* __restrict__ p = jp_col(sm, ch);
    float v[8], f[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[k * JP_LD];
    dct8<false>(v, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = w[ch][k] * f[k];
    dct8<true>(f, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * JP_LD] = o[k];
  }
  __syncthreads();
  {
    float o[3][8];
    jp_rows_inv(sm, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float uy = o[0][e], ub = o[1][e], ur = o[2][e];
      const float r0 = 0.299f * uy, r1 = -0.168736f * ub, r2 = 0.5f * ur;
      const float g0 = 0.587f * uy, g1 = -0.331264f * ub, g2 = -0.418688f * ur;
      const float b0 = 0.114f * uy, b1 = 0.5f * ub, b2 = -0.081312f * ur;
      o[0][e] = (r0 + r1) + r2;
      o[1][e] = (g0 + g1) + g2;
      o[2][e] = (b0 + b1) + b2;
    }
    jp_rows_put(sm, o);
  }
  __syncthreads();
  float a1[4], a2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) a1[e] = a2[e] = 0.f;
  bool bad = false;
  for (int qi = 0; qi < 2; ++qi) {
    const JpPos p = jp_pos(threadIdx.x, qi, ty0, tx0, S);
    if (!p.in) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[4];
      ldv<4>(sm + ch * JP_PLANE + p.row * JP_LD + p.col, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bad |= !__builtin_isfinite(v[e]);
        a1[e] += fabsf(v[e]);
        a2[e] = fmaf(v[e], v[e], a2[e]);
      }
      st4<VEC>(op + ch * hw + p.off, v);
    }
  }
  if (bad && nonfinite) nonfinite[n] = 1;
  block_slot_store<2>(lane_sum<4>(a1), lane_sum<4>(a2), part);
}

}  // namespace mia

using namespace mia;

// the checks shared by the two JPEG entry points: the plane geometry and N
#define MIA_CHECK_JPEG(N, S)                                                               \
  MIA_CHECK_ARG((S) >= 8 && (S) % 8 == 0, "S must be a multiple of 8, >= 8");              \
  MIA_CHECK_ARG((int64_t)3 * (S) * (S) < (1LL << 31), "3·S² must be below 2^31");          \
  MIA_CHECK_IMAGES(N, (int64_t)3 * (S) * (S))

extern "C" int mia_jpeg_roundtrip(const float* x, float* y, const float* qtab, int N, int S,
                                  void* stream) {
  MIA_CHECK_ARG(x && y && qtab, "null x / y / qtab");
  MIA_CHECK_JPEG(N, S);
  const int64_t len = (int64_t)N * 3 * S * S;
  MIA_CHECK_ARG(disjoint({words(x, len), words(y, len), words(qtab, 128)}),
                "x, y and qtab must be distinct buffers");
  const bool vec = vec_ok(S, {x, y});
  const int tiles_x = (S + JP_TX - 1) / JP_TX, tiles_y = (S + JP_TY - 1) / JP_TY;
  const dim3 grid(tiles_x * tiles_y, N);
  return launch2("jpeg_roundtrip_kernel", jpeg_roundtrip_kernel<true>,
                 jpeg_roundtrip_kernel<false>, vec, grid, 0, (hipStream_t)stream, x, y, qtab, S,
                 tiles_x);
}

extern "C" int mia_jpeg_bwd_norms(const float* x, const float* g, float* gx, const float* qtab,
                                  float* l1, float* l2sq, int N, int S, int* nonfinite,
                                  void* stream) {
  MIA_CHECK_ARG(x && g && gx && qtab, "null x / g / gx / qtab");
  MIA_CHECK_JPEG(N, S);
  const int64_t len = (int64_t)N * 3 * S * S;
  MIA_CHECK_ARG(disjoint({words(x, len), words(g, len), words(gx, len), words(qtab, 128)}),
                "x, g, gx and qtab must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = vec_ok(S, {x, g, gx});
  const int tiles_x = (S + JP_TX - 1) / JP_TX, tiles_y = (S + JP_TY - 1) / JP_TY;
  const dim3 grid(tiles_x * tiles_y, N);
  return launch_norms(l1, l2sq, grid, N, st, [&](float* part) {
    return launch2("jpeg_bwd_norms_kernel", jpeg_bwd_norms_kernel<true>,
                   jpeg_bwd_norms_kernel<false>, vec, grid, 0, st, x, g, gx, qtab, part, S,
                   tiles_x, nonfinite);
  });
}
