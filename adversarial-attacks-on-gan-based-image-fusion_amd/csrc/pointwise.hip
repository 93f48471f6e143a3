// HBM-bound kernels of the attack step (gfx950): bias/act, StyledConv backward front, ToRGB,
// upfirdn2d, max/avg pooling, MSE pieces, image layout changes and the PGD sign-project step.
// Feature maps are NHWC and moved in 16-byte vectors (4 fp32 / 8 fp16|bf16 per lane).
#include "mia_common.h"

namespace mia {

constexpr int TPB = 256;

static inline int blocks_for(int64_t n, int per_block = TPB, int cap = 1 << 20) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

// ---------------------------------------------------------------------------------------------
// K4 forward, standalone: y = lrelu(x + nw·noise[p] + b[c])·√2 (rosinality FusedLeakyReLU after
// NoiseInjection). The fused path writes `pre` from the conv epilogue instead.
template <typename T>
__global__ void bias_act_fwd_kernel(const T* __restrict__ x, const float* __restrict__ noise,
                                    float nw, const float* __restrict__ bias, T* __restrict__ y,
                                    int64_t nvec, int C, int HW) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * TPB) {
    const int64_t e0 = i * V;
    const int c0 = (int)(e0 % C);
    const int p = (int)((e0 / C) % HW);
    VT v = ((const VT*)x)[i];
    const float nz = noise ? nw * noise[p] : 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = from_f<T>(lrelu_s2(to_f(v[e]) + nz + (bias ? bias[c0 + e] : 0.f)));
    ((VT*)y)[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// StyledConv backward front. One block = a run of pixels of one image, all channels.
template <typename T>
__global__ void bias_act_bwd_kernel(const T* __restrict__ g_a, const T* __restrict__ pre,
                                    const float* __restrict__ noise, float nw,
                                    const float* __restrict__ bias, const float* __restrict__ demod,
                                    T* __restrict__ gy, float* __restrict__ qpart, int H, int W,
                                    int C, int unshuffle, int from_act, int pix_per_block) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  __shared__ float red[TPB * 8];
  const int n = blockIdx.y;
  const int HW = H * W;
  const int tpp = C / V;             // threads per pixel (≤ 256)
  const int ppp = TPB / tpp;         // pixels per pass
  const int t = threadIdx.x;
  const int chunk = t % tpp, sub = t / tpp;
  const int c0 = chunk * V;
  float qa[V];
#pragma unroll
  for (int e = 0; e < V; ++e) qa[e] = 0.f;
  float dm[V], bs[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    dm[e] = demod[(size_t)n * C + c0 + e];
    bs[e] = bias ? bias[c0 + e] : 0.f;
  }
  const int p_begin = blockIdx.x * pix_per_block;
  const int p_end = min(p_begin + pix_per_block, HW);
  if (sub < ppp) {
    for (int p = p_begin + sub; p < p_end; p += ppp) {
      const size_t off = ((size_t)n * HW + p) * C + c0;
      const VT ga = *(const VT*)(g_a + off);
      const VT pr = *(const VT*)(pre + off);
      const float nz = noise ? nw * noise[p] : 0.f;
      VT o;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float pin = to_f(pr[e]);
        const float gr = lrelu_s2_grad(pin);  // same sign for pre and act = lrelu(pre)·√2
        const float pv = from_act ? pin / gr : pin;
        const float gp = to_f(ga[e]) * gr;
        qa[e] += gp * (pv - nz - bs[e]);
        o[e] = from_f<T>(gp * dm[e]);
      }
      size_t ooff = off;
      if (unshuffle) {
        const int y = p / W, x = p - (p / W) * W;
        const int R = H / 2, Rw = W / 2;
        const int ph = ((y & 1) << 1) | (x & 1);
        ooff = (((size_t)n * R + (y >> 1)) * Rw + (x >> 1)) * (4 * C) + ph * C + c0;
      }
      *(VT*)(gy + ooff) = o;
    }
  }
  // reduce q over the `ppp` pixel lanes sharing a channel chunk
#pragma unroll
  for (int e = 0; e < V; ++e) red[t * V + e] = qa[e];
  __syncthreads();
  if (sub == 0) {
    for (int s = 1; s < ppp; ++s)
#pragma unroll
      for (int e = 0; e < V; ++e) qa[e] += red[(s * tpp + chunk) * V + e];
    // the block's partial into its slot (blockIdx.x); red_finish adds the slots in order
#pragma unroll
    for (int e = 0; e < V; ++e)
      red_store(qpart, gridDim.x, gridDim.y * C, 0, blockIdx.x, n * C + c0 + e, qa[e]);
  }
}

// ---------------------------------------------------------------------------------------------
// Blur of the up-sampling StyledConv (rosinality Blur: upfirdn2d, k = [1,3,3,1]⊗[1,3,3,1]/64·4,
// pad (1,1)) applied to the transposed-conv output T (N, 2R+1, 2R+1, C), fused with the
// demodulation scale, noise injection and bias: pre = demod·blur(T) + nw·noise + b.
__constant__ float kBlur4[4] = {0.25f, 0.75f, 0.75f, 0.25f};

// Both directions are the same separable 4-tap FIR (factor-2 up-sampling phases). A thread owns a
// 2-wide × 2·KQ-tall output strip of one 8-channel (16-byte) vector and streams down the 2·KQ+3
// input rows it needs: each row is loaded once (5 vectors), filtered horizontally into the strip's
// 2 columns, and accumulated into the ≤ 4 output rows it feeds; an output row is stored as soon as
// its 4th input row has been added (≈ 3.4 loads per output instead of 16 for a direct 4×4 FIR).
//   forward : out = pre (N,2R,2R,C),    in = T  (N,2R+1,2R+1,C), input row of output row 0 is −1
//   backward: out = gT (N,2R+1,2R+1,C), in = gy (N,2R,2R,C),     input row of output row 0 is −2
// (the adjoint flips the taps; the kernel is symmetric so the weights are the same).
// input rows in flight per thread: 4 (round 6; 2 before: fp32 forward / adjoint −1.5 / −3.9 %,
// fp16 −2.9 / −2.5 % per generator pass, still 2 waves per SIMD; profiles/r06_blur_pf_ab.txt)
#ifndef MIA_BLUR_PF
#define MIA_BLUR_PF 4
#endif
#ifndef MIA_BLUR_KQ  // output rows per strip / 2 (swept 2 … 6: profiles/r06_blur_kq_sweep.txt)
#define MIA_BLUR_KQ 4
#endif
constexpr int kBlurKQ = MIA_BLUR_KQ;
static __device__ __attribute__((aligned(16))) uint4 g_blur_zero[1];  // zero page (out-of-range taps)


// V consecutive fp32 values (V = 8 or 4) with 16-byte loads
template <int V>
__device__ __forceinline__ void load8f_or_4(const float* p, float (&v)[V]) {
#pragma unroll
  for (int q = 0; q < V / 4; ++q) {
    const f32x4 t = *(const f32x4*)(p + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
  }
}

template <typename T, bool FWD, bool NOISE>
__global__ __launch_bounds__(256) void blur4_strip_kernel(
    const T* __restrict__ in, T* __restrict__ out, const float* __restrict__ demod,
    const float* __restrict__ noise, float nw, const float* __restrict__ bias, int N, int R, int C,
    int act_out) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  constexpr int KQ = kBlurKQ, OR = 2 * KQ, IR = 2 * KQ + 3;
  const int Hin = FWD ? 2 * R + 1 : 2 * R;
  const int Hout = FWD ? 2 * R : 2 * R + 1;
  const int Q = (Hout + 1) / 2;     // 2-wide columns per row
  const int SY = (Hout + OR - 1) / OR;  // strips per column
  const int off0 = FWD ? -1 : -2;
  const int nc = C / V;
  const int64_t total = (int64_t)N * SY * Q * nc;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    int cv, qx, sy, n;
    if (total < (1LL << 31)) {  // 32-bit divisions: a third of the 64-bit ones' VALU
      unsigned u = (unsigned)i;
      cv = (int)(u % (unsigned)nc);
      u /= (unsigned)nc;
      qx = (int)(u % (unsigned)Q);
      u /= (unsigned)Q;
      sy = (int)(u % (unsigned)SY);
      n = (int)(u / (unsigned)SY);
    } else {
      cv = (int)(i % nc);
      const int64_t r1 = i / nc;
      qx = (int)(r1 % Q);
      const int64_t r2 = r1 / Q;
      sy = (int)(r2 % SY);
      n = (int)(r2 / SY);
    }
    const int x0 = 2 * qx + off0, y0 = sy * OR + off0;
    const int oy0 = sy * OR, ox0 = 2 * qx;
    float dm[V], bs[V];
    if (FWD) {
      load8f_or_4(demod + (size_t)n * C + cv * V, dm);
      if (bias) {
        load8f_or_4(bias + cv * V, bs);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) bs[e] = 0.f;
      }
    }
    const T* base = in + (size_t)n * Hin * Hin * C + cv * V;
    T* obase = out + (size_t)n * Hout * Hout * C + cv * V;
    // noise of the whole strip up front: a global load issued between the pipelined row loads
    // would force a vmcnt(0) drain (the counter retires in order)
    // (NOISE is a template flag so that no branch separates these loads from the row loads)
    float nzs[OR][2];
#pragma unroll
    for (int a = 0; a < OR; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        nzs[a][b] = NOISE ? noise[min(oy0 + a, Hout - 1) * Hout + min(ox0 + b, Hout - 1)] : 0.f;
    float acc[OR][2][V];
    // software pipeline: rows rl+1 … rl+PF are in flight while row rl is filtered. Loads are
    // unconditional: an out-of-range tap reads the zero page (round 6: the address is selected,
    // not the loaded values zeroed; with 32-bit index math −1 … −4 %, profiles/r06_blur_v2_ab.txt).
    int xc[5];
    bool xv[5];
#pragma unroll
    for (int lc = 0; lc < 5; ++lc) {
      const int xx = x0 + lc;
      xv[lc] = xx >= 0 && xx < Hin;
      xc[lc] = min(max(xx, 0), Hin - 1);
    }
    constexpr int PF = MIA_BLUR_PF;  // input rows in flight ahead of the one being filtered
    VT nx[PF][5];
    // out-of-range taps load the zero page (the address is selected, not the 8 loaded values)
    auto src = [&](int yy, int lc) {
      const bool ok = yy >= 0 && yy < Hin && xv[lc];
      return ok ? base + ((size_t)yy * Hin + xc[lc]) * C : (const T*)g_blur_zero;
    };
#pragma unroll
    for (int q = 0; q < PF; ++q)
#pragma unroll
      for (int lc = 0; lc < 5; ++lc) nx[q][lc] = *(const VT*)src(y0 + q, lc);
#pragma unroll
    for (int rl = 0; rl < IR; ++rl) {
      const int yy = y0 + rl;
      VT v[5];
#pragma unroll
      for (int lc = 0; lc < 5; ++lc) {
        v[lc] = nx[0][lc];
#pragma unroll
        for (int q = 0; q + 1 < PF; ++q) nx[q][lc] = nx[q + 1][lc];
      }
      if (rl + PF < IR) {
#pragma unroll
        for (int lc = 0; lc < 5; ++lc) nx[PF - 1][lc] = *(const VT*)src(yy + PF, lc);
      }
      float h[2][V];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < V; ++e)
          h[b][e] = kBlur4[0] * to_f(v[b][e]) + kBlur4[1] * to_f(v[b + 1][e]) +
                    kBlur4[2] * to_f(v[b + 2][e]) + kBlur4[3] * to_f(v[b + 3][e]);
#pragma unroll
      for (int a = 0; a < OR; ++a) {
        const int j = rl - a;
        if (j < 0 || j > 3) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int e = 0; e < V; ++e)
            acc[a][b][e] = (j == 0 ? 0.f : acc[a][b][e]) + kBlur4[j] * h[b][e];
        if (j != 3) continue;
        // output row a is complete
        const int oy = oy0 + a;
        if (oy >= Hout) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int ox = ox0 + b;
          if (ox >= Hout) continue;
          VT o;
          const float nz = nw * nzs[a][b];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            float r = acc[a][b][e];
            if (FWD) {
              r = r * dm[e] + nz + bs[e];
              if (act_out) r = lrelu_s2(r);
            }
            o[e] = from_f<T>(r);
          }
          *(VT*)(obase + ((size_t)oy * Hout + ox) * C) = o;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// upfirdn2d on fp32 NCHW planes with a separable kernel (rosinality op/upfirdn2d semantics).
__device__ __forceinline__ float upfir_at(const float* __restrict__ x, int H, int W, int oy, int ox,
                                          const float* kf, int kt, int up, int down, int pad0) {
  float acc = 0.f;
  for (int jy = 0; jy < kt; ++jy) {
    const int ty = oy * down + jy - pad0;
    if (ty < 0 || ty % up) continue;
    const int iy = ty / up;
    if (iy >= H) continue;
    for (int jx = 0; jx < kt; ++jx) {
      const int tx = ox * down + jx - pad0;
      if (tx < 0 || tx % up) continue;
      const int ix = tx / up;
      if (ix >= W) continue;
      acc += x[iy * W + ix] * kf[jy] * kf[jx];
    }
  }
  return acc;
}

struct Taps8 { float k[8]; };

__global__ void upfirdn2d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int planes,
                                     int H, int W, int Ho, int Wo, Taps8 kf, int kt, int up,
                                     int down, int pad0) {
  const int64_t total = (int64_t)planes * Ho * Wo;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int ox = (int)(i % Wo);
    const int oy = (int)((i / Wo) % Ho);
    const int64_t pl = i / ((int64_t)Wo * Ho);
    y[i] = upfir_at(x + pl * H * W, H, W, oy, ox, kf.k, kt, up, down, pad0);
  }
}

__global__ void upfirdn2d_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                     int planes, int H, int W, int Ho, int Wo, Taps8 kf, int kt,
                                     int up, int down, int pad0) {
  const int64_t total = (int64_t)planes * H * W;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int ix = (int)(i % W);
    const int iy = (int)((i / W) % H);
    const int64_t pl = i / ((int64_t)W * H);
    const float* g = gy + pl * Ho * Wo;
    float acc = 0.f;
    for (int jy = 0; jy < kt; ++jy) {
      const int sy = iy * up + pad0 - jy;  // = oy*down
      if (sy < 0 || sy % down) continue;
      const int oy = sy / down;
      if (oy >= Ho) continue;
      for (int jx = 0; jx < kt; ++jx) {
        const int sx = ix * up + pad0 - jx;
        if (sx < 0 || sx % down) continue;
        const int ox = sx / down;
        if (ox >= Wo) continue;
        acc += g[oy * Wo + ox] * kf.k[jy] * kf.k[jx];
      }
    }
    gx[i] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// ToRGB (1x1 modulated conv without demod) + bias + up-sampled skip. A group of `tpp` lanes owns a
// pixel (each lane a slice of channels); the 3 partial dot products are reduced by shuffles.
__constant__ float kUp4[4] = {0.25f, 0.75f, 0.75f, 0.25f};  // [1,3,3,1]/sum · 2 (per axis)

// The ToRGB skip term upfirdn2d(skip, [1,3,3,1]⊗[1,3,3,1]/16·4, up = 2, pad = (2, 1)) at output
// (y, x): the two taps per axis that land on input samples, added in upfir_at's order with its
// expression (bit-identical), loaded unconditionally from clamped addresses (out-of-range taps
// zeroed) so that the four loads issue back-to-back.
__device__ __forceinline__ float skip_up2(const float* __restrict__ sk, int Hs, int Ws, int y,
                                          int x) {
  const int py = y & 1, px = x & 1;
  const int iy0 = (y - 2 + py) >> 1, ix0 = (x - 2 + px) >> 1;
  float v[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int iy = iy0 + a, ix = ix0 + b;
      const bool ok = iy >= 0 && iy < Hs && ix >= 0 && ix < Ws;
      const float t = sk[min(max(iy, 0), Hs - 1) * Ws + min(max(ix, 0), Ws - 1)];
      v[a][b] = ok ? t : 0.f;
    }
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc += v[a][b] * kUp4[py + 2 * a] * kUp4[px + 2 * b];
  return acc;
}

template <typename T, int LV>
__global__ __launch_bounds__(TPB) void torgb_fwd_kernel(const T* __restrict__ pre, const float* __restrict__ s,
                                 const float* __restrict__ wr, const float* __restrict__ bias,
                                 const float* __restrict__ skip, float* __restrict__ rgb, int H,
                                 int W, int Cin, int tpp, int cpt, int pix_per_block, int act_in) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  constexpr int U = 4;  // pixels in flight per lane group (U independent 16-B loads per lane)
  extern __shared__ float wm[];  // [3][Cin]
  const int n = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * Cin; i += TPB) wm[i] = wr[i] * s[(size_t)n * Cin + (i % Cin)];
  __syncthreads();
  const int HW = H * W, Hs = H / 2, Ws = W / 2;
  const int t = threadIdx.x;
  const int g = t % tpp, sub = t / tpp, ppp = TPB / tpp;
  const int p_begin = blockIdx.x * pix_per_block;
  const int p_end = min(p_begin + pix_per_block, HW);
  const T* img = pre + (size_t)n * HW * Cin;
  // The 12 sums (pixel u, channel c) of a lane group sit in 16 slots k = 4u + c (c = 3 empty) and
  // are reduce-scattered over the group's lanes: at level o (o = 1, 2, 4, 8 while o < tpp) a lane
  // keeps the half of its slots picked by lane bit o and adds the partner's copy of that half —
  // 8 + 4 + 2 + 1 shuffles instead of a butterfly's 12 per level; levels o ≥ 16 add the one slot
  // left. Each addition pairs the same lanes in the same level order as a butterfly (own +
  // partner), so every sum is bit-identical to it. LV = min(4, log2 tpp) scatter levels (a
  // template parameter: levels skipped at run time would keep both versions of the slots live).
  // This lane ends with slots base … base + nsl − 1.
  constexpr int nsl = 16 >> LV;
  int base = 0;
#pragma unroll
  for (int lv = 0; lv < LV; ++lv)
    if (g & (1 << lv)) base += 8 >> lv;
  const bool owner = g < 16;  // lanes g ≥ 16 hold copies of lanes g − 16's slots
  auto skip_at = [&](int k, int pb) {  // the up-sampled skip term of slot k (0 if none)
    const int u = k >> 2, c = k & 3, p = pb + u * ppp + sub;
    if (!skip || !owner || c == 3 || p >= p_end) return 0.f;
    const int y = p / W, x = p - (p / W) * W;
    return skip_up2(skip + ((size_t)n * 3 + c) * Hs * Ws, Hs, Ws, y, x);
  };
  for (int pb = p_begin; pb < p_end; pb += ppp * U) {
    // the skip terms first: their loads overlap the channel loads instead of following the
    // reduction (the first 4 of the lane's slots: all of them from tpp = 4 on)
    float skv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) skv[i] = i < nsl ? skip_at(base + i, pb) : 0.f;
    float a[U][3];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u][0] = a[u][1] = a[u][2] = 0.f;
    for (int cc = 0; cc < cpt; ++cc) {
      const int c0 = (g + cc * tpp) * V;
      VT v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {  // clamped, unconditional: the U loads issue back-to-back
        const int p = min(pb + u * ppp + sub, p_end - 1);
        v[u] = *(const VT*)(img + (size_t)p * Cin + c0);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float w0 = wm[c0 + e], w1 = wm[Cin + c0 + e], w2 = wm[2 * Cin + c0 + e];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float x = act_in ? lrelu_s2(to_f(v[u][e])) : to_f(v[u][e]);
          // fused explicitly: a contractible a += x·w may be left unfused when the vectorizer
          // pairs the products, which made the 2-byte outputs depend on code generation
          a[u][0] = __builtin_fmaf(x, w0, a[u][0]);
          a[u][1] = __builtin_fmaf(x, w1, a[u][1]);
          a[u][2] = __builtin_fmaf(x, w2, a[u][2]);
        }
      }
    }
    float sl[16];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      sl[4 * u] = a[u][0];
      sl[4 * u + 1] = a[u][1];
      sl[4 * u + 2] = a[u][2];
      sl[4 * u + 3] = 0.f;
    }
#pragma unroll
    for (int lv = 0; lv < LV; ++lv) {
      const int o = 1 << lv, h = 8 >> lv;
      const bool hi = (g & o) != 0;
#pragma unroll
      for (int i = 0; i < h; ++i) {
        // (the asm hides that both operands are loads of sl: folding the selects into one
        // select-indexed load would keep sl in memory as a 16-way compare chain)
        float x = sl[i], y = sl[h + i];
        asm volatile("" : "+v"(x), "+v"(y));
        const float keep = hi ? y : x, send = hi ? x : y;
        sl[i] = keep + __shfl_xor(send, o, 64);
      }
    }
    for (int o = 16; o < tpp; o <<= 1) sl[0] += __shfl_xor(sl[0], o, 64);
#pragma unroll
    for (int i = 0; i < nsl; ++i) {
      const int k = base + i, u = k >> 2, c = k & 3;
      const int p = pb + u * ppp + sub;
      if (!owner || c == 3 || p >= p_end) continue;
      float r = bias[c];
      r += sl[i];
      if (skip) r += i < 4 ? skv[i] : skip_at(k, pb);
      rgb[((size_t)n * 3 + c) * HW + p] = r;
    }
  }
}

// FRONT: the ToRGB feeds the topmost StyledConv, whose activation gradient is this ToRGB's alone;
// then also run that conv's backward front (as mia_bias_act_bwd(from_act) would): g_a is written
// as gy = g·lrelu'(a)·demod and q[n][c] += g·lrelu'(a)·(pre − nw·noise − b).
struct TorgbFront {
  const float* demod;
  const float* noise;
  float nw;
  const float* bias;
  float* q;
};

template <typename T, bool FRONT>
__global__ void torgb_bwd_kernel(const float* __restrict__ grgb, const T* __restrict__ pre,
                                 const float* __restrict__ s, const float* __restrict__ wr,
                                 T* __restrict__ g_a, float* __restrict__ part_out, int H, int W,
                                 int Cin, int accumulate, int pix_per_block, int act_in,
                                 TorgbFront fr) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  extern __shared__ float sh[];  // wr [3][Cin], s [Cin], partials [TPB/tpp][Cin] (× 2 if FRONT)
  const int n = blockIdx.y;
  float* w3 = sh;
  float* sn = sh + 3 * Cin;
  float* part = sh + 4 * Cin;
  for (int i = threadIdx.x; i < 3 * Cin; i += TPB) w3[i] = wr[i];
  for (int i = threadIdx.x; i < Cin; i += TPB) sn[i] = s[(size_t)n * Cin + i];
  __syncthreads();
  const int HW = H * W;
  const int nch = Cin / V;                // chunks per pixel
  const int tpp = nch < TPB ? nch : TPB;  // one chunk per thread
  const int ppp = TPB / tpp;
  const int t = threadIdx.x;
  const int chunk = t % tpp, sub = t / tpp;
  const int c0 = chunk * V;
  float acc[V], qa[V], dm[V], bs[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = qa[e] = 0.f;
  if (FRONT) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      dm[e] = fr.demod[(size_t)n * Cin + c0 + e];
      bs[e] = fr.bias ? fr.bias[c0 + e] : 0.f;
    }
  }
  const int p_begin = blockIdx.x * pix_per_block;
  const int p_end = min(p_begin + pix_per_block, HW);
  if (sub < ppp) {
    for (int p = p_begin + sub; p < p_end; p += ppp) {
      const float g0 = grgb[((size_t)n * 3 + 0) * HW + p];
      const float g1 = grgb[((size_t)n * 3 + 1) * HW + p];
      const float g2 = grgb[((size_t)n * 3 + 2) * HW + p];
      const size_t off = ((size_t)n * HW + p) * Cin + c0;
      const VT pr = *(const VT*)(pre + off);
      VT ga;
      if (accumulate) ga = *(const VT*)(g_a + off);
      const float nz = (FRONT && fr.noise) ? fr.nw * fr.noise[p] : 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int c = c0 + e;
        const float u = g0 * w3[c] + g1 * w3[Cin + c] + g2 * w3[2 * Cin + c];
        acc[e] += (act_in ? lrelu_s2(to_f(pr[e])) : to_f(pr[e])) * u;
        float gv = sn[c] * u + (accumulate ? to_f(ga[e]) : 0.f);
        if (FRONT) {  // stored activation a = pr (act_in NONE)
          const float a = to_f(pr[e]);
          const float gr = lrelu_s2_grad(a);
          const float gp = gv * gr;
          qa[e] += gp * (a * lrelu_s2_inv_grad(a) - nz - bs[e]);
          gv = gp * dm[e];
        }
        ga[e] = from_f<T>(gv);
      }
      *(VT*)(g_a + off) = ga;
    }
  }
  float* partq = part + ppp * Cin;
  if (sub < ppp) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      part[sub * Cin + c0 + e] = acc[e];
      if (FRONT) partq[sub * Cin + c0 + e] = qa[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < Cin; c += TPB) {
    float sum = 0.f, sq = 0.f;
    for (int sb = 0; sb < ppp; ++sb) {
      sum += part[sb * Cin + c];
      if (FRONT) sq += partq[sb * Cin + c];
    }
    // the block's partials into its slot (blockIdx.x): gs (quantity 0) and q (1)
    red_store(part_out, gridDim.x, gridDim.y * Cin, 0, blockIdx.x, n * Cin + c, sum);
    if (FRONT) red_store(part_out, gridDim.x, gridDim.y * Cin, 1, blockIdx.x, n * Cin + c, sq);
  }
}

// ---------------------------------------------------------------------------------------------
// MaxPool 2x2 stride 2 (NHWC), PyTorch semantics incl. ceil_mode and first-max tie rule.
// One thread per 2×2 window and 16-byte channel vector. All loads are unconditional (coordinates
// clamped into the image; a clamped duplicate is excluded by its validity flag), so they issue
// back-to-back instead of each behind its own branch and vmcnt(0).
template <typename T>
__global__ void maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H,
                                    int W, int C, int Ho, int Wo) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  const int nc = C / V;
  const int64_t total = (int64_t)N * Ho * Wo * nc;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int cv = (int)(i % nc);
    const int64_t pix = i / nc;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((int64_t)Wo * Ho));
    const int y0 = 2 * oy, x0 = 2 * ox;
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const T* b = x + (size_t)n * H * W * C + cv * V;
    const VT v[4] = {*(const VT*)(b + ((size_t)y0 * W + x0) * C),
                     *(const VT*)(b + ((size_t)y0 * W + x1) * C),
                     *(const VT*)(b + ((size_t)y1 * W + x0) * C),
                     *(const VT*)(b + ((size_t)y1 * W + x1) * C)};
    const bool ok[4] = {true, x0 + 1 < W, y0 + 1 < H, x0 + 1 < W && y0 + 1 < H};
    VT best = v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (!ok[k]) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float fv = to_f(v[k][e]), fb = to_f(best[e]);
        if (fv > fb || fv != fv) best[e] = v[k][e];  // first max wins; NaN propagates
      }
    }
    *(VT*)(y + pix * C + cv * V) = best;
  }
}

// Backward per window: the window's gradient goes to its first-max position; the tap-MSE term
// tap_coef·(x − t) and the ReLU mask (x > 0) of the layer below are fused. Windows beyond
// (Ho, Wo) (floor mode, odd size) only carry the tap/mask terms.
template <typename T, bool TAP>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gout,
                                    T* __restrict__ gin, int N, int H, int W, int C, int Ho, int Wo,
                                    const T* __restrict__ tap_t, float tap_coef, int mask) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  const int nc = C / V;
  const int WY = (H + 1) / 2, WX = (W + 1) / 2;
  const int64_t total = (int64_t)N * WY * WX * nc;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int cv = (int)(i % nc);
    const int64_t w = i / nc;
    const int wx = (int)(w % WX);
    const int wy = (int)((w / WX) % WY);
    const int n = (int)(w / ((int64_t)WX * WY));
    const int y0 = 2 * wy, x0 = 2 * wx;
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const size_t off[4] = {((size_t)y0 * W + x0) * C, ((size_t)y0 * W + x1) * C,
                           ((size_t)y1 * W + x0) * C, ((size_t)y1 * W + x1) * C};
    const bool ok[4] = {true, x0 + 1 < W, y0 + 1 < H, x0 + 1 < W && y0 + 1 < H};
    const size_t img = (size_t)n * H * W * C + cv * V;
    const bool pooled = wy < Ho && wx < Wo;
    const VT go = *(const VT*)(gout + (((size_t)n * Ho + min(wy, Ho - 1)) * Wo + min(wx, Wo - 1)) * C +
                               cv * V);
    VT xv[4], tv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = *(const VT*)(x + img + off[k]);
    if (TAP) {
#pragma unroll
      for (int k = 0; k < 4; ++k) tv[k] = *(const VT*)(tap_t + img + off[k]);
    }
    int bpos[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float bv = to_f(xv[0][e]);
      bpos[e] = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float fv = to_f(xv[k][e]);
        if (ok[k] && (fv > bv || fv != fv)) { bv = fv; bpos[e] = k; }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!ok[k]) continue;
      VT o;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xf = to_f(xv[k][e]);
        float r = (pooled && bpos[e] == k) ? to_f(go[e]) : 0.f;
        if (TAP) r += tap_coef * (xf - to_f(tv[k][e]));
        if (mask && !(xf > 0.f)) r = 0.f;
        o[e] = from_f<T>(r);
      }
      *(VT*)(gin + img + off[k]) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// avg_pool2d(k, stride k) on fp32 NCHW planes and its backward.
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int planes,
                                   int H, int W, int k) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)planes * Ho * Wo;
  const float inv = 1.f / (float)(k * k);
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int ox = (int)(i % Wo);
    const int oy = (int)((i / Wo) % Ho);
    const int64_t pl = i / ((int64_t)Wo * Ho);
    const float* xp = x + pl * H * W + (size_t)oy * k * W + ox * k;
    float acc = 0.f;
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) acc += xp[dy * W + dx];
    y[i] = acc * inv;
  }
}

__global__ void avgpool_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                   int planes, int H, int W, int k, int accumulate) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)planes * H * W;
  const float inv = 1.f / (float)(k * k);
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int ix = (int)(i % W);
    const int iy = (int)((i / W) % H);
    const int64_t pl = i / ((int64_t)W * H);
    const int oy = iy / k, ox = ix / k;
    float v = (oy < Ho && ox < Wo) ? gy[pl * Ho * Wo + oy * Wo + ox] * inv : 0.f;
    if (accumulate) v += gx[i];
    gx[i] = v;
  }
}

// NCHW fp32 (N,3,S,S) → avg_pool(pf) → NHWC (N,S/pf,S/pf,cpad) in T, channels ≥ 3 zero.
template <typename T>
__global__ void image_to_nhwc_kernel(const float* __restrict__ x, T* __restrict__ y, int N, int S,
                                     int pf, int cpad) {
  const int R = S / pf;
  const int64_t total = (int64_t)N * R * R * cpad;
  const float inv = 1.f / (float)(pf * pf);
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int c = (int)(i % cpad);
    const int64_t pix = i / cpad;
    const int xo = (int)(pix % R);
    const int yo = (int)((pix / R) % R);
    const int n = (int)(pix / ((int64_t)R * R));
    float v = 0.f;
    if (c < 3) {
      const float* xp = x + (((size_t)n * 3 + c) * S + (size_t)yo * pf) * S + xo * pf;
      for (int dy = 0; dy < pf; ++dy)
        for (int dx = 0; dx < pf; ++dx) v += xp[dy * S + dx];
      v *= inv;
    }
    y[i] = from_f<T>(v);
  }
}

// The same with cpad a multiple of the 16-byte vector (the product's CPAD = 8): one thread per
// output pixel, its 3 planes' loads coalesced across the wave and its cpad channels written as
// whole 16-byte vectors (the element-per-thread form wrote 2- / 4-byte scalars at 1.8 TB/s).
// Same sums in the same order: bit-identical.
template <typename T>
__global__ __launch_bounds__(TPB) void image_to_nhwc_vec_kernel(const float* __restrict__ x,
                                                                T* __restrict__ y, int N, int S,
                                                                int pf, int cpad) {
  typedef typename Vec<T>::type VT;
  constexpr int V = Vec<T>::N;
  const int R = S / pf;
  const int64_t total = (int64_t)N * R * R;
  const float inv = 1.f / (float)(pf * pf);
  for (int64_t pix = blockIdx.x * (int64_t)TPB + threadIdx.x; pix < total;
       pix += (int64_t)gridDim.x * TPB) {
    const int xo = (int)(pix % R);
    const int yo = (int)((pix / R) % R);
    const int n = (int)(pix / ((int64_t)R * R));
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* xp = x + (((size_t)n * 3 + c) * S + (size_t)yo * pf) * S + xo * pf;
      float a = 0.f;
      for (int dy = 0; dy < pf; ++dy)
        for (int dx = 0; dx < pf; ++dx) a += xp[dy * S + dx];
      v[c] = a * inv;
    }
    T* out = y + pix * cpad;
    for (int q = 0; q < cpad / V; ++q) {
      VT o;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int ch = q * V + e;
        o[e] = from_f<T>(ch < 3 ? v[ch < 3 ? ch : 0] : 0.f);
      }
      *(VT*)(out + q * V) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MSE pieces (K10).
template <typename T>
__global__ void mse_sum_kernel(const T* __restrict__ a, const T* __restrict__ b,
                               float* __restrict__ part, int64_t len, float coef) {
  const int n = blockIdx.y;
  const T* pa = a + (size_t)n * len;
  const T* pb = b + (size_t)n * len;
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float d = to_f(pa[i]) - to_f(pb[i]);
    acc += d * d;
  }
  __shared__ float red[TPB / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < TPB / 64; ++w) s += red[w];
    red_store(part, gridDim.x, gridDim.y, 0, blockIdx.x, n, coef * s);  // the block's slot
  }
}

__global__ void mse_grad_f32_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                    float* __restrict__ g, int64_t len, float coef, int accumulate) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    float v = coef * (a[i] - b[i]);
    if (accumulate) v += g[i];
    g[i] = v;
  }
}

template <typename T>
__global__ void tap_grad_kernel(const T* __restrict__ a, const T* __restrict__ t, T* __restrict__ g,
                                int64_t len, float coef, int mask) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float av = to_f(a[i]);
    float v = coef * (av - to_f(t[i]));
    if (mask && !(av > 0.f)) v = 0.f;
    g[i] = from_f<T>(v);
  }
}

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
// memory. Every kernel here runs on a (slots, N) grid, block (b, n) striding over image n alone:
// an image's partial sums — and so its norms — depend on its own plane size only, never on the
// other images of the call. V = 4: 16-byte accesses (plane % 4 == 0 and 16-byte aligned bases,
// decided by the launcher); V = 1: scalar.
template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&v)[V]) {
  if (V == 4) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = t[e];
  } else {
    v[0] = p[0];
  }
}

template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[V]) {
  if (V == 4) {
    f32x4 t;
#pragma unroll
    for (int e = 0; e < V; ++e) t[e] = v[e];
    *(f32x4*)p = t;
  } else {
    p[0] = v[0];
  }
}

// the V per-lane accumulators of a thread, pairwise (a chain of 2 additions instead of 4)
template <int V>
__device__ __forceinline__ float lane_sum(const float (&a)[V]) {
  return V == 4 ? (a[0] + a[1]) + (a[2] + a[3]) : a[0];
}

// The block's sums of s0 (quantity 0) and s1 (quantity 1, NQ = 2) into its slot blockIdx.x of
// image blockIdx.y: wave butterflies, then the 4 wave sums in wave order (mse_sum_kernel's tree).
// Every thread of the block must call it. part = nullptr: no quantity was asked for.
template <int NQ>
__device__ __forceinline__ void block_slot_store(float s0, float s1, float* __restrict__ part) {
  __shared__ float red[2][TPB / 64];
  s0 = wave_sum(s0);
  if (NQ > 1) s1 = wave_sum(s1);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s0;
    if (NQ > 1) red[1][threadIdx.x >> 6] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0 && part) {
    float t0 = 0.f, t1 = 0.f;
    for (int w = 0; w < TPB / 64; ++w) {
      t0 += red[0][w];
      if (NQ > 1) t1 += red[1][w];
    }
    red_store(part, gridDim.x, gridDim.y, 0, blockIdx.x, blockIdx.y, t0);
    if (NQ > 1) red_store(part, gridDim.x, gridDim.y, 1, blockIdx.x, blockIdx.y, t1);
  }
}

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

// PixelNorm of the mapping network input (rosinality PixelNorm): y = x / sqrt(mean(x²) + eps)
// over each row of `cols` values; one block per row.
__global__ void pixel_norm_kernel(const float* __restrict__ x, float* __restrict__ y, int cols,
                                  float eps) {
  const float* xr = x + (size_t)blockIdx.x * cols;
  float* yr = y + (size_t)blockIdx.x * cols;
  float acc = 0.f;
  for (int i = threadIdx.x; i < cols; i += TPB) acc += xr[i] * xr[i];
  __shared__ float red[TPB / 64];
  __shared__ float inv;
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < TPB / 64; ++w) s += red[w];
    inv = rsqrtf(s / (float)cols + eps);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cols; i += TPB) yr[i] = xr[i] * inv;
}

// Truncation trick (rosinality Generator.forward): out = mean + psi·(w − mean), mean broadcast
// over rows.
__global__ void truncate_kernel(const float* __restrict__ w, const float* __restrict__ mean,
                                float psi, float* __restrict__ out, int64_t len, int cols) {
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < len; i += (int64_t)gridDim.x * TPB) {
    const float m = mean[i % cols];
    out[i] = m + psi * (w[i] - m);
  }
}

__global__ void repeat_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                              int64_t bytes, int count) {
  const int64_t total = bytes * count;
  for (int64_t i = blockIdx.x * (int64_t)TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB)
    dst[i] = src[i % bytes];
}

}  // namespace mia

using namespace mia;

#define MIA_LAUNCH(kern, grid, block, shmem, ...)                                  \
  do {                                                                             \
    hipLaunchKernelGGL(kern, grid, block, shmem, (hipStream_t)stream, __VA_ARGS__); \
    return check_launch(#kern);                                                    \
  } while (0)

extern "C" int mia_bias_act_fwd(const void* x, const float* noise, float noise_w,
                                const float* bias, void* y, int N, int H, int W, int C, int dtype,
                                void* stream) {
  MIA_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0, "C must be a multiple of the vector width");
  const int64_t nvec = (int64_t)N * H * W * C / V;
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(bias_act_fwd_kernel<T>, dim3(blocks_for(nvec, TPB, 65536)), dim3(TPB), 0,
                 (const T*)x, noise, noise_w, bias, (T*)y, nvec, C, H * W));
  return MIA_OK;
}

extern "C" int mia_bias_act_bwd(const void* g_a, const void* pre, const float* noise,
                                float noise_w, const float* bias, const float* demod, void* gy,
                                float* q, int N, int H, int W, int C, int unshuffle, int from_act,
                                int dtype, void* stream) {
  MIA_CHECK_ARG(g_a && pre && demod && gy && q, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0 && C / V <= TPB && (TPB % (C / V)) == 0, "C/V must divide 256");
  MIA_CHECK_ARG(!unshuffle || (H % 2 == 0 && W % 2 == 0), "unshuffle needs even H, W");
  const int HW = H * W;
  const int ppp = TPB / (C / V);
  const int ppb = ppp * 16;
  dim3 grid((HW + ppb - 1) / ppb, N);
  RedQ r;
  int rc = red_begin(r, q, nullptr, nullptr, grid.x, N * C, (hipStream_t)stream);
  if (rc != MIA_OK) return rc;
  MIA_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL(bias_act_bwd_kernel<T>, grid, dim3(TPB), 0, (hipStream_t)stream,
                         (const T*)g_a, (const T*)pre, noise, noise_w, bias, demod, (T*)gy, r.part,
                         H, W, C, unshuffle, from_act, ppb));
  rc = check_launch("bias_act_bwd_kernel");
  return rc != MIA_OK ? rc : red_finish(r, (hipStream_t)stream);
}

extern "C" int mia_upconv_blur_fwd(const void* t, void* pre, const float* demod,
                                   const float* noise, float noise_w, const float* bias, int N,
                                   int R, int C, int act_out, int dtype, void* stream) {
  MIA_CHECK_ARG(t && pre && demod && N > 0 && R > 0, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0, "C must be a multiple of the vector width");
  const int SY = (2 * R + 2 * kBlurKQ - 1) / (2 * kBlurKQ);
  const int64_t total = (int64_t)N * SY * R * (C / V);
  MIA_DISPATCH_DTYPE(dtype, T,
      if (noise) {
        MIA_LAUNCH((blur4_strip_kernel<T, true, true>), dim3(blocks_for(total, TPB, 65536)),
                   dim3(TPB), 0, (const T*)t, (T*)pre, demod, noise, noise_w, bias, N, R, C,
                   act_out);
      } else {
        MIA_LAUNCH((blur4_strip_kernel<T, true, false>), dim3(blocks_for(total, TPB, 65536)),
                   dim3(TPB), 0, (const T*)t, (T*)pre, demod, noise, noise_w, bias, N, R, C,
                   act_out);
      });
  return MIA_OK;
}

extern "C" int mia_upconv_blur_bwd(const void* gy, void* gt, int N, int R, int C, int dtype,
                                   void* stream) {
  MIA_CHECK_ARG(gy && gt && N > 0 && R > 0, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0, "C must be a multiple of the vector width");
  const int SY = (2 * R + 1 + 2 * kBlurKQ - 1) / (2 * kBlurKQ);
  const int64_t total = (int64_t)N * SY * (R + 1) * (C / V);
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH((blur4_strip_kernel<T, false, false>), dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0,
                 (const T*)gy, (T*)gt, nullptr, nullptr, 0.f, nullptr, N, R, C, 0));
  return MIA_OK;
}

static int make_taps(const float* k1d, int ktaps, Taps8* kf) {
  if (ktaps < 1 || ktaps > 8) return mia::set_error("upfirdn2d: 1..8 taps");
  for (int j = 0; j < 8; ++j) kf->k[j] = 0.f;
  for (int j = 0; j < ktaps; ++j) kf->k[j] = k1d[ktaps - 1 - j];  // flipped (correlation form)
  return MIA_OK;
}

extern "C" int mia_upfirdn2d_fwd(const float* x, float* y, int planes, int H, int W,
                                 const float* k1d, int ktaps, int up, int down, int pad0, int pad1,
                                 void* stream) {
  MIA_CHECK_ARG(x && y && k1d && up >= 1 && down >= 1, "bad args");
  Taps8 kf;
  if (make_taps(k1d, ktaps, &kf)) return MIA_EINVAL;
  const int Ho = (H * up + pad0 + pad1 - ktaps) / down + 1;
  const int Wo = (W * up + pad0 + pad1 - ktaps) / down + 1;
  MIA_CHECK_ARG(Ho > 0 && Wo > 0, "empty output");
  const int64_t total = (int64_t)planes * Ho * Wo;
  MIA_LAUNCH(upfirdn2d_fwd_kernel, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, x, y, planes,
             H, W, Ho, Wo, kf, ktaps, up, down, pad0);
}

extern "C" int mia_upfirdn2d_bwd(const float* gy, float* gx, int planes, int H, int W,
                                 const float* k1d, int ktaps, int up, int down, int pad0, int pad1,
                                 void* stream) {
  MIA_CHECK_ARG(gy && gx && k1d && up >= 1 && down >= 1, "bad args");
  Taps8 kf;
  if (make_taps(k1d, ktaps, &kf)) return MIA_EINVAL;
  const int Ho = (H * up + pad0 + pad1 - ktaps) / down + 1;
  const int Wo = (W * up + pad0 + pad1 - ktaps) / down + 1;
  MIA_CHECK_ARG(Ho > 0 && Wo > 0, "empty output");
  const int64_t total = (int64_t)planes * H * W;
  MIA_LAUNCH(upfirdn2d_bwd_kernel, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, gy, gx,
             planes, H, W, Ho, Wo, kf, ktaps, up, down, pad0);
}

// the ToRGB forward with lv = min(4, log2 tpp) reduce-scatter levels (each lane keeps 16 >> lv
// of the lane group's 16 sum slots)
template <typename T>
static int launch_torgb_fwd(dim3 grid, size_t sh, const T* pre, const float* style,
                            const float* wr, const float* bias, const float* skip, float* rgb,
                            int H, int W, int Cin, int tpp, int cpt, int ppb, int act_in,
                            hipStream_t st) {
  const int lv = tpp >= 16 ? 4 : tpp == 8 ? 3 : tpp == 4 ? 2 : tpp == 2 ? 1 : 0;
  auto fn = lv == 4 ? torgb_fwd_kernel<T, 4> : lv == 3 ? torgb_fwd_kernel<T, 3>
          : lv == 2 ? torgb_fwd_kernel<T, 2> : lv == 1 ? torgb_fwd_kernel<T, 1>
                    : torgb_fwd_kernel<T, 0>;
  hipLaunchKernelGGL(fn, grid, dim3(TPB), sh, st, pre, style, wr, bias, skip, rgb, H, W, Cin, tpp,
                     cpt, ppb, act_in);
  return check_launch("torgb_fwd_kernel");
}

extern "C" int mia_torgb_fwd(const void* pre, const float* style, const float* wr,
                             const float* bias, const float* skip, float* rgb, int N, int H, int W,
                             int Cin, int act_in, int dtype, void* stream) {
  MIA_CHECK_ARG(pre && style && wr && bias && rgb, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(Cin % V == 0, "Cin must be a multiple of the vector width");
  int nch = Cin / V;
  int tpp = 1;
  while (tpp * 2 <= nch && tpp * 2 <= 64) tpp *= 2;
  MIA_CHECK_ARG(nch % tpp == 0, "Cin/V must be a power of two times tpp");
  const int cpt = nch / tpp;
  const int ppb = (TPB / tpp) * 16;  // 4 passes of U = 4 pixels per lane group
  dim3 grid((H * W + ppb - 1) / ppb, N);
  const size_t sh = 3 * Cin * sizeof(float);
  MIA_DISPATCH_DTYPE(dtype, T,
      return launch_torgb_fwd<T>(grid, sh, (const T*)pre, style, wr, bias, skip, rgb, H, W, Cin,
                                 tpp, cpt, ppb, act_in, (hipStream_t)stream));
  return MIA_OK;
}

extern "C" int mia_torgb_bwd(const float* g_rgb, const void* pre, const float* style,
                             const float* wr, void* g_a, float* gs, int N, int H, int W, int Cin,
                             int accumulate, int act_in, int dtype, void* stream) {
  MIA_CHECK_ARG(g_rgb && pre && style && wr && g_a && gs, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(Cin % V == 0 && Cin / V <= TPB && TPB % (Cin / V) == 0, "Cin/V must divide 256");
  const int ppp = TPB / (Cin / V);
  const int ppb = ppp * 16;
  dim3 grid((H * W + ppb - 1) / ppb, N);
  const size_t sh = (4 * Cin + (size_t)ppp * Cin) * sizeof(float);
  MIA_CHECK_ARG(sh <= 64 * 1024, "LDS budget");
  const TorgbFront fr{};
  RedQ r;
  int rc = red_begin(r, gs, nullptr, nullptr, grid.x, N * Cin, (hipStream_t)stream);
  if (rc != MIA_OK) return rc;
  MIA_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL((torgb_bwd_kernel<T, false>), grid, dim3(TPB), sh, (hipStream_t)stream,
                         g_rgb, (const T*)pre, style, wr, (T*)g_a, r.part, H, W, Cin, accumulate,
                         ppb, act_in, fr));
  rc = check_launch("torgb_bwd_kernel");
  return rc != MIA_OK ? rc : red_finish(r, (hipStream_t)stream);
}

extern "C" int mia_torgb_bwd_front(const float* g_rgb, const void* act, const float* style,
                                   const float* wr, void* gy, float* gs, int N, int H, int W,
                                   int Cin, const float* demod, const float* noise, float noise_w,
                                   const float* bias, float* q, int dtype, void* stream) {
  MIA_CHECK_ARG(g_rgb && act && style && wr && gy && gs && demod && q, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(Cin % V == 0 && Cin / V <= TPB && TPB % (Cin / V) == 0, "Cin/V must divide 256");
  const int ppp = TPB / (Cin / V);
  const int ppb = ppp * 16;
  dim3 grid((H * W + ppb - 1) / ppb, N);
  const size_t sh = (4 * Cin + 2 * (size_t)ppp * Cin) * sizeof(float);
  MIA_CHECK_ARG(sh <= 64 * 1024, "LDS budget");
  const TorgbFront fr{demod, noise, noise_w, bias, q};
  RedQ r;
  int rc = red_begin(r, gs, q, nullptr, grid.x, N * Cin, (hipStream_t)stream);
  if (rc != MIA_OK) return rc;
  MIA_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL((torgb_bwd_kernel<T, true>), grid, dim3(TPB), sh, (hipStream_t)stream,
                         g_rgb, (const T*)act, style, wr, (T*)gy, r.part, H, W, Cin, 0, ppb,
                         MIA_ACT_NONE, fr));
  rc = check_launch("torgb_bwd_kernel");
  return rc != MIA_OK ? rc : red_finish(r, (hipStream_t)stream);
}

static inline int pool_out(int H, int ceil_mode) { return ceil_mode ? (H + 1) / 2 : H / 2; }

extern "C" int mia_maxpool2_fwd(const void* x, void* y, int N, int H, int W, int C, int ceil_mode,
                                int dtype, void* stream) {
  MIA_CHECK_ARG(x && y && H >= 2 && W >= 2, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0, "C must be a multiple of the vector width");
  const int Ho = pool_out(H, ceil_mode), Wo = pool_out(W, ceil_mode);
  const int64_t total = (int64_t)N * Ho * Wo * (C / V);
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(maxpool2_fwd_kernel<T>, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0,
                 (const T*)x, (T*)y, N, H, W, C, Ho, Wo));
  return MIA_OK;
}

extern "C" int mia_maxpool2_bwd(const void* x, const void* g_out, void* g_in, int N, int H, int W,
                                int C, int ceil_mode, const void* tap_t, float tap_coef, int mask,
                                int dtype, void* stream) {
  MIA_CHECK_ARG(x && g_out && g_in && H >= 2 && W >= 2, "bad args");
  const int V = dtype == MIA_F32 ? 4 : 8;
  MIA_CHECK_ARG(C % V == 0, "C must be a multiple of the vector width");
  const int Ho = pool_out(H, ceil_mode), Wo = pool_out(W, ceil_mode);
  const int64_t total = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / V);
  MIA_DISPATCH_DTYPE(dtype, T,
      if (tap_t) {
        MIA_LAUNCH((maxpool2_bwd_kernel<T, true>), dim3(blocks_for(total, TPB, 65536)), dim3(TPB),
                   0, (const T*)x, (const T*)g_out, (T*)g_in, N, H, W, C, Ho, Wo, (const T*)tap_t,
                   tap_coef, mask);
      } else {
        MIA_LAUNCH((maxpool2_bwd_kernel<T, false>), dim3(blocks_for(total, TPB, 65536)), dim3(TPB),
                   0, (const T*)x, (const T*)g_out, (T*)g_in, N, H, W, C, Ho, Wo, (const T*)tap_t,
                   tap_coef, mask);
      });
  return MIA_OK;
}

extern "C" int mia_avgpool_fwd(const float* x, float* y, int planes, int H, int W, int k,
                               void* stream) {
  MIA_CHECK_ARG(x && y && k >= 1 && H >= k && W >= k, "bad args");
  const int64_t total = (int64_t)planes * (H / k) * (W / k);
  MIA_LAUNCH(avgpool_fwd_kernel, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, x, y, planes,
             H, W, k);
}

extern "C" int mia_avgpool_bwd(const float* gy, float* gx, int planes, int H, int W, int k,
                               int accumulate, void* stream) {
  MIA_CHECK_ARG(gy && gx && k >= 1 && H >= k && W >= k, "bad args");
  const int64_t total = (int64_t)planes * H * W;
  MIA_LAUNCH(avgpool_bwd_kernel, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, gy, gx, planes,
             H, W, k, accumulate);
}

extern "C" int mia_image_to_nhwc(const float* x, void* y, int N, int S, int pf, int cpad,
                                 int dtype, void* stream) {
  MIA_CHECK_ARG(x && y && pf >= 1 && S % pf == 0 && cpad >= 3, "bad args");
  const int R = S / pf;
  const int64_t total = (int64_t)N * R * R * cpad;
  const int V = dtype == MIA_F32 ? 4 : 8;
  if (cpad % V == 0) {
    const int64_t pixels = (int64_t)N * R * R;
    MIA_DISPATCH_DTYPE(dtype, T,
        MIA_LAUNCH(image_to_nhwc_vec_kernel<T>, dim3(blocks_for(pixels, TPB, 65536)), dim3(TPB),
                   0, x, (T*)y, N, S, pf, cpad));
  }
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(image_to_nhwc_kernel<T>, dim3(blocks_for(total, TPB, 65536)), dim3(TPB), 0, x,
                 (T*)y, N, S, pf, cpad));
  return MIA_OK;
}

extern "C" int mia_mse_sum(const void* a, const void* b, float* loss, int n, int64_t len,
                           float coef, int dtype, void* stream) {
  MIA_CHECK_ARG(a && b && loss && n > 0 && len > 0, "bad args");
  dim3 grid(blocks_for(len, TPB, 1024), n);
  RedQ r;
  int rc = red_begin(r, loss, nullptr, nullptr, grid.x, n, (hipStream_t)stream);
  if (rc != MIA_OK) return rc;
  MIA_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL(mse_sum_kernel<T>, grid, dim3(TPB), 0, (hipStream_t)stream, (const T*)a,
                         (const T*)b, r.part, len, coef));
  rc = check_launch("mse_sum_kernel");
  return rc != MIA_OK ? rc : red_finish(r, (hipStream_t)stream);
}

extern "C" int mia_mse_grad_f32(const float* a, const float* b, float* g, int64_t len, float coef,
                                int accumulate, void* stream) {
  MIA_CHECK_ARG(a && b && g && len > 0, "bad args");
  MIA_LAUNCH(mse_grad_f32_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, a, b, g, len,
             coef, accumulate);
}

extern "C" int mia_tap_grad(const void* a, const void* t, void* g, int64_t len, float coef,
                            int mask, int dtype, void* stream) {
  MIA_CHECK_ARG(a && t && g && len > 0, "bad args");
  MIA_DISPATCH_DTYPE(dtype, T,
      MIA_LAUNCH(tap_grad_kernel<T>, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, (const T*)a,
                 (const T*)t, (T*)g, len, coef, mask));
  return MIA_OK;
}

extern "C" int mia_mse_fwd_bwd(const void* a, const void* b, float* loss, void* g, int n,
                               int64_t len, float coef_loss, float coef_grad, int accumulate,
                               int dtype, void* stream) {
  MIA_CHECK_ARG(a && b && (loss || g) && n > 0 && len > 0, "bad args");
  MIA_CHECK_ARG(!g || dtype == MIA_F32 || !accumulate,
                "accumulating gradient is fp32 only (mia_mse_grad_f32)");
  if (loss) {
    const int rc = mia_mse_sum(a, b, loss, n, len, coef_loss, dtype, stream);
    if (rc != MIA_OK) return rc;
  }
  if (!g) return MIA_OK;
  if (dtype == MIA_F32)
    return mia_mse_grad_f32((const float*)a, (const float*)b, (float*)g, (int64_t)n * len,
                            coef_grad, accumulate, stream);
  return mia_tap_grad(a, b, g, (int64_t)n * len, coef_grad, 0, dtype, stream);
}

// The shape checks of the launchers that read the pooled gradients per image element
// (image_grad / pgd_update / grad_assemble; mia_grad_assemble_norms makes the same ones): the
// kernels index g_vgg as [n][y / pf][x / pf][c < 3] of cpad channels and g_enc as
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

// (slots, N) grid of the per-image passes: ≤ 1024 slots of TPB threads, each moving V floats
static inline dim3 image_grid(int64_t plane, int V, int N) {
  return dim3(blocks_for(plane / V, TPB, 1024), N);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define MIA_CHECK_IMAGES(N, plane)                                                      \
  MIA_CHECK_ARG((N) > 0 && (N) <= 65535, "N must be in 1 … 65535");                     \
  MIA_CHECK_ARG((plane) > 0 && (plane) < (1LL << 31), "plane must be in 1 … 2^31 − 1")

extern "C" int mia_grad_assemble_norms(const float* x, const float* x0, const void* g_vgg,
                                       const float* g_enc, float* g, float* l1, float* l2sq,
                                       int N, int S, int pf, int cpad, int enc_res,
                                       float coef_img, float scale, int* nonfinite, int dtype,
                                       void* stream) {
  MIA_CHECK_ARG(x && x0 && g, "null x / x0 / g");
  MIA_CHECK_ARG(S > 0 && S <= 16384, "S must be in 1 … 16384");
  const int64_t plane = (int64_t)3 * S * S;
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(pf >= 1 && S % pf == 0, "pf must divide S");
  MIA_CHECK_ARG(!g_vgg || cpad >= 3, "cpad must be >= 3");
  MIA_CHECK_ARG(!g_enc || (enc_res >= 1 && S % enc_res == 0), "enc_res must divide S");
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_F16 || dtype == MIA_BF16, "unsupported dtype");
  if (!g_enc) enc_res = S;  // unused, but the kernel divides by S / enc_res
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g);
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  RedQ r;
  int rc = red_begin(r, l1, l2sq, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  MIA_DISPATCH_DTYPE(dtype, T,
      if (vec) {
        hipLaunchKernelGGL((grad_assemble_norms_kernel<T, 4>), grid, dim3(TPB), 0, st, x, x0,
                           (const T*)g_vgg, g_enc, g, r.part, plane, S, pf, cpad, enc_res,
                           coef_img, scale, nonfinite);
      } else {
        hipLaunchKernelGGL((grad_assemble_norms_kernel<T, 1>), grid, dim3(TPB), 0, st, x, x0,
                           (const T*)g_vgg, g_enc, g, r.part, plane, S, pf, cpad, enc_res,
                           coef_img, scale, nonfinite);
      });
  rc = check_launch("grad_assemble_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
}

extern "C" int mia_l2_step(float* x, const float* x0, const float* g, const float* gnorm2sq,
                           float* dsq_out, int N, int64_t plane, float a, int* nonfinite,
                           void* stream) {
  MIA_CHECK_ARG(x && x0 && g && gnorm2sq && dsq_out, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(a > 0.f, "the step a must be > 0");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g);
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  RedQ r;
  int rc = red_begin(r, dsq_out, nullptr, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(l2_step_kernel<4>, grid, dim3(TPB), 0, st, x, x0, g, gnorm2sq, r.part,
                       plane, a, nonfinite);
  else
    hipLaunchKernelGGL(l2_step_kernel<1>, grid, dim3(TPB), 0, st, x, x0, g, gnorm2sq, r.part,
                       plane, a, nonfinite);
  rc = check_launch("l2_step_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
}

extern "C" int mia_l2_project(float* x, const float* x0, const float* dsq, int N, int64_t plane,
                              float e, float lo, float hi, void* stream) {
  MIA_CHECK_ARG(x && x0 && dsq, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(e > 0.f && lo <= hi, "need e > 0 and lo <= hi");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(x0);
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  if (vec)
    MIA_LAUNCH(l2_project_kernel<4>, grid, dim3(TPB), 0, x, x0, dsq, plane, e, lo, hi);
  MIA_LAUNCH(l2_project_kernel<1>, grid, dim3(TPB), 0, x, x0, dsq, plane, e, lo, hi);
}

extern "C" int mia_mi_update(float* x, const float* x0, const float* g, const float* l1, float* m,
                             int N, int64_t plane, float mu, float a, float e, float lo, float hi,
                             int* nonfinite, void* stream) {
  MIA_CHECK_ARG(x && x0 && g && l1 && m, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(mu >= 0.f && a > 0.f && e > 0.f && lo <= hi,
                "need mu >= 0, a > 0, e > 0 and lo <= hi");
  const bool vec =
      plane % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g) && aligned16(m);
  const dim3 grid = image_grid(plane, vec ? 4 : 1, N);
  if (vec)
    MIA_LAUNCH(mi_update_kernel<4>, grid, dim3(TPB), 0, x, x0, g, l1, m, plane, mu, a, e, lo, hi,
               nonfinite);
  MIA_LAUNCH(mi_update_kernel<1>, grid, dim3(TPB), 0, x, x0, g, l1, m, plane, mu, a, e, lo, hi,
             nonfinite);
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
  const bool vec = W % 4 == 0 && aligned16(g) && aligned16(gs);
  const int tiles_x = (W + TI_T - 1) / TI_T, tiles_y = (H + TI_T - 1) / TI_T;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
  const void* fn = vec ? (const void*)ti_smooth_norms_kernel<4>
                       : (const void*)ti_smooth_norms_kernel<1>;
  if (const int rc = ensure_dyn_lds(fn, TiGeom(TI_MAXK).floats * 4); rc != MIA_OK) return rc;
  const int lds = TiGeom(K).floats * 4;
  RedQ r;
  int rc = red_begin(r, l1, l2sq, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(ti_smooth_norms_kernel<4>, grid, dim3(TPB), lds, st, g, gs, taps, K,
                       r.part, C, H, W, tiles_x, tiles_y, nonfinite);
  else
    hipLaunchKernelGGL(ti_smooth_norms_kernel<1>, grid, dim3(TPB), lds, st, g, gs, taps, K,
                       r.part, C, H, W, tiles_x, tiles_y, nonfinite);
  rc = check_launch("ti_smooth_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
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
  MIA_CHECK_ARG(!di_overlap(a, b, (int64_t)(N) * (C) * (S) * (S)),                            \
                "the input and the output must be distinct buffers")

static inline bool di_overlap(const float* a, const float* b, int64_t len) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)len * sizeof(float);
  return pa < pb ? pb - pa < bytes : pa - pb < bytes;
}

extern "C" int mia_di_resize_pad(const float* x, float* y, int N, int C, int S, int rnd, int top,
                                 int left, void* stream) {
  MIA_CHECK_DI(x, y, N, C, S, rnd, top, left);
  const bool vec = S % 4 == 0 && aligned16(x) && aligned16(y);
  const int tiles_x = (S + DI_TX - 1) / DI_TX, tiles_y = (S + DI_TY - 1) / DI_TY;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
  if (vec)
    MIA_LAUNCH(di_resize_pad_kernel<true>, grid, dim3(TPB), 0, x, y, C, S, rnd, top, left,
               tiles_x, tiles_y);
  MIA_LAUNCH(di_resize_pad_kernel<false>, grid, dim3(TPB), 0, x, y, C, S, rnd, top, left, tiles_x,
             tiles_y);
}

extern "C" int mia_di_resize_pad_bwd_norms(const float* g, float* gx, float* l1, float* l2sq,
                                           int N, int C, int S, int rnd, int top, int left,
                                           int* nonfinite, void* stream) {
  MIA_CHECK_DI(g, gx, N, C, S, rnd, top, left);
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = S % 4 == 0 && aligned16(g) && aligned16(gx);
  const int tiles_x = (S + DI_TX - 1) / DI_TX, tiles_y = (S + DI_TY - 1) / DI_TY;
  const dim3 grid(C * tiles_x * tiles_y, N);
  RedQ r;
  int rc = red_begin(r, l1, l2sq, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(di_resize_pad_bwd_norms_kernel<true>, grid, dim3(TPB), 0, st, g, gx,
                       r.part, C, S, rnd, top, left, tiles_x, tiles_y, nonfinite);
  else
    hipLaunchKernelGGL(di_resize_pad_bwd_norms_kernel<false>, grid, dim3(TPB), 0, st, g, gx,
                       r.part, C, S, rnd, top, left, tiles_x, tiles_y, nonfinite);
  rc = check_launch("di_resize_pad_bwd_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
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
  MIA_CHECK_ARG(!di_overlap(x, y, len) && !(m && di_overlap(m, y, len)),
                "the inputs and the output must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(y) && (!m || aligned16(m));
  const dim3 grid = image_grid(plane + 3, 4, N);
  if (vec) MIA_LAUNCH(si_transform_kernel<true>, grid, dim3(TPB), 0, x, m, y, plane, c, s);
  MIA_LAUNCH(si_transform_kernel<false>, grid, dim3(TPB), 0, x, m, y, plane, c, s);
}

extern "C" int mia_si_accumulate_norms(const float* g, float* acc, float* l1, float* l2sq, int N,
                                       int64_t plane, float w, int first, float div,
                                       int* nonfinite, void* stream) {
  MIA_CHECK_ARG(g && acc, "null g / acc");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(si_scale_ok(w), "w must be 2^-i with 0 <= i < MIA_SI_MAX_SCALES");
  MIA_CHECK_ARG(__builtin_isfinite(div) && div >= 1.f, "div must be finite and >= 1");
  MIA_CHECK_ARG(!di_overlap(g, acc, (int64_t)N * plane), "g and acc must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = plane % 4 == 0 && aligned16(g) && aligned16(acc);
  const dim3 grid = image_grid(plane + 3, 4, N);
  RedQ r;
  int rc = red_begin(r, l1, l2sq, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(si_accumulate_norms_kernel<true>, grid, dim3(TPB), 0, st, g, acc, r.part,
                       plane, w, first != 0, div, nonfinite);
  else
    hipLaunchKernelGGL(si_accumulate_norms_kernel<false>, grid, dim3(TPB), 0, st, g, acc, r.part,
                       plane, w, first != 0, div, nonfinite);
  rc = check_launch("si_accumulate_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
}

extern "C" int mia_vt_neighbor(const float* x, const float* m, float* y, int N, int64_t plane,
                               float c, float r, uint64_t seed, uint32_t image0, uint32_t step,
                               uint32_t sample, void* stream) {
  MIA_CHECK_ARG(x && y, "null x / y");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG((uint64_t)image0 + (uint64_t)N <= (1ULL << 32), "image0 + N must be <= 2^32");
  MIA_CHECK_ARG(__builtin_isfinite(c), "c must be finite");
  MIA_CHECK_ARG(__builtin_isfinite(r) && r >= 0.f, "r must be finite and >= 0");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(x, y, len) && !(m && di_overlap(m, y, len)),
                "the inputs and the output must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(y) && (!m || aligned16(m));
  const dim3 grid = image_grid(plane + 3, 4, N);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  if (vec)
    MIA_LAUNCH(vt_neighbor_kernel<true>, grid, dim3(TPB), 0, x, m, y, plane, c, r, k0, k1, image0,
               step, sample);
  MIA_LAUNCH(vt_neighbor_kernel<false>, grid, dim3(TPB), 0, x, m, y, plane, c, r, k0, k1, image0,
             step, sample);
}

extern "C" int mia_vt_combine_norms(const float* g, const float* gv, float* v, float* gt,
                                    float* l1, int N, int64_t plane, int* nonfinite,
                                    void* stream) {
  MIA_CHECK_ARG(g && v && gt, "null g / v / gt");
  MIA_CHECK_IMAGES(N, plane);
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(g, v, len) && !di_overlap(g, gt, len) && !di_overlap(v, gt, len) &&
                    !(gv && (di_overlap(gv, g, len) || di_overlap(gv, v, len) ||
                             di_overlap(gv, gt, len))),
                "g, gv, v and gt must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = plane % 4 == 0 && aligned16(g) && aligned16(v) && aligned16(gt) &&
                   (!gv || aligned16(gv));
  const dim3 grid = image_grid(plane + 3, 4, N);
  RedQ r;
  int rc = red_begin(r, l1, nullptr, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(vt_combine_norms_kernel<true>, grid, dim3(TPB), 0, st, g, gv, v, gt,
                       r.part, plane, nonfinite);
  else
    hipLaunchKernelGGL(vt_combine_norms_kernel<false>, grid, dim3(TPB), 0, st, g, gv, v, gt,
                       r.part, plane, nonfinite);
  rc = check_launch("vt_combine_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
}

extern "C" int mia_spsa_probe(const float* x, float* yp, float* ym, int N, int64_t plane, float d,
                              float lo, float hi, uint64_t seed, uint32_t image0, uint32_t step,
                              uint32_t sample, void* stream) {
  MIA_CHECK_ARG(x && yp && ym, "null x / yp / ym");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG((uint64_t)image0 + (uint64_t)N <= (1ULL << 32), "image0 + N must be <= 2^32");
  MIA_CHECK_ARG(__builtin_isfinite(d) && d > 0.f, "d must be finite and > 0");
  MIA_CHECK_ARG(lo <= hi, "need lo <= hi");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(x, yp, len) && !di_overlap(x, ym, len) && !di_overlap(yp, ym, len),
                "x, yp and ym must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(yp) && aligned16(ym);
  const dim3 grid = image_grid(plane + 3, 4, N);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  if (vec)
    MIA_LAUNCH(spsa_probe_kernel<true>, grid, dim3(TPB), 0, x, yp, ym, plane, d, lo, hi, k0, k1,
               image0, step, sample);
  MIA_LAUNCH(spsa_probe_kernel<false>, grid, dim3(TPB), 0, x, yp, ym, plane, d, lo, hi, k0, k1,
             image0, step, sample);
}

extern "C" int mia_spsa_accumulate_norms(float* acc, const float* fp, const float* fm, float* l1,
                                         float* l2sq, int N, int64_t plane, float s, uint64_t seed,
                                         uint32_t image0, uint32_t step, uint32_t sample, int first,
                                         float div, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(acc && fp && fm, "null acc / fp / fm");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG((uint64_t)image0 + (uint64_t)N <= (1ULL << 32), "image0 + N must be <= 2^32");
  MIA_CHECK_ARG(__builtin_isfinite(s) && s > 0.f, "s must be finite and > 0");
  MIA_CHECK_ARG(__builtin_isfinite(div) && div > 0.f, "div must be finite and > 0");
  // acc: N·plane floats; fp, fm: N floats each
  const auto inside = [](const float* a, int64_t la, const float* b, int64_t lb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < (uintptr_t)la * sizeof(float) : pa - pb < (uintptr_t)lb * sizeof(float);
  };
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!inside(acc, len, fp, N) && !inside(acc, len, fm, N) && !inside(fp, N, fm, N),
                "acc, fp and fm must be distinct buffers");
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = plane % 4 == 0 && aligned16(acc);
  const dim3 grid = image_grid(plane + 3, 4, N);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  RedQ r;
  int rc = red_begin(r, l1, l2sq, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  if (vec)
    hipLaunchKernelGGL(spsa_accumulate_norms_kernel<true>, grid, dim3(TPB), 0, st, acc, fp, fm,
                       r.part, plane, s, k0, k1, image0, step, sample, first != 0, div, nonfinite);
  else
    hipLaunchKernelGGL(spsa_accumulate_norms_kernel<false>, grid, dim3(TPB), 0, st, acc, fp, fm,
                       r.part, plane, s, k0, k1, image0, step, sample, first != 0, div, nonfinite);
  rc = check_launch("spsa_accumulate_norms_kernel");
  return rc != MIA_OK ? rc : red_finish(r, st);
}

// Block rows of mia_uap_accumulate's grid: 1 = the loop form (a thread walks all N images and
// stores its group), > 1 = the image-split form on integer atomics. Both are exact; DESIGN.md
// records the A/B behind the default.
#ifndef MIA_UAP_SPLIT
#define MIA_UAP_SPLIT 1
#endif

static inline bool byte_overlap(const void* a, int64_t la, const void* b, int64_t lb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb ? pb - pa < (uintptr_t)la : pa - pb < (uintptr_t)lb;
}

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
  const int64_t gb = (int64_t)N * plane * 4, ab = plane * 8, lb = (int64_t)N * 4;
  MIA_CHECK_ARG(!byte_overlap(g, gb, acc, ab) && !byte_overlap(l1, lb, acc, ab) &&
                    !byte_overlap(g, gb, l1, lb) &&
                    !(nonfinite && (byte_overlap(nonfinite, lb, acc, ab) ||
                                    byte_overlap(nonfinite, lb, g, gb) ||
                                    byte_overlap(nonfinite, lb, l1, lb))),
                "g, l1, acc and nonfinite must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(g) && aligned16(acc);
  const int rows = MIA_UAP_SPLIT < N ? MIA_UAP_SPLIT : N;
  const dim3 grid(blocks_for((plane + 3) / 4, TPB), rows);
  if (rows > 1 && first) {
    const int rc = mia_memset(acc, 0, ab, stream);
    if (rc != MIA_OK) return rc;
  }
  if (vec)
    MIA_LAUNCH(uap_accumulate_kernel<true>, grid, dim3(TPB), 0, g, l1, (long long*)acc, N, plane,
               first != 0, nonfinite);
  MIA_LAUNCH(uap_accumulate_kernel<false>, grid, dim3(TPB), 0, g, l1, (long long*)acc, N, plane,
             first != 0, nonfinite);
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
  const int64_t xb = (int64_t)N * plane * 4, db = plane * 4, ab = plane * 8;
  MIA_CHECK_ARG(!(acc && byte_overlap(delta, db, acc, ab)), "delta and acc must be distinct");
  if (N > 0)
    MIA_CHECK_ARG(!byte_overlap(x, xb, x0, xb) && !byte_overlap(x, xb, delta, db) &&
                      !byte_overlap(x0, xb, delta, db) &&
                      !(acc && (byte_overlap(x, xb, acc, ab) || byte_overlap(x0, xb, acc, ab))),
                  "delta, acc, x and x0 must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(delta) && (!acc || aligned16(acc)) &&
                   (N == 0 || (aligned16(x) && aligned16(x0)));
  const dim3 grid(blocks_for((plane + 3) / 4, TPB));
  if (vec)
    MIA_LAUNCH(uap_step_kernel<true>, grid, dim3(TPB), 0, delta, (const long long*)acc, x, x0, N,
               plane, a, e, lo, hi);
  MIA_LAUNCH(uap_step_kernel<false>, grid, dim3(TPB), 0, delta, (const long long*)acc, x, x0, N,
             plane, a, e, lo, hi);
}

extern "C" int mia_apgd_update(float* x, float* x_old, const float* x0, const float* g,
                               const float* eta, int N, int64_t plane, float a, float e, float lo,
                               float hi, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(x && x_old && x0 && g && eta, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  MIA_CHECK_ARG(a > 0.f && a <= 1.f, "the momentum weight a must be in (0, 1]");
  MIA_CHECK_ARG(e > 0.f && __builtin_isfinite(e) && lo <= hi, "need a finite e > 0 and lo <= hi");
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(x, x_old, len) && !di_overlap(x, x0, len) && !di_overlap(x, g, len) &&
                    !di_overlap(x_old, x0, len) && !di_overlap(x_old, g, len),
                "x, x_old, x0 and g must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(x_old) && aligned16(x0) &&
                   aligned16(g);
  const dim3 grid = image_grid(plane + 3, 4, N);
  if (vec)
    MIA_LAUNCH(apgd_update_kernel<true>, grid, dim3(TPB), 0, x, x_old, x0, g, eta, plane, a, e, lo,
               hi, nonfinite);
  MIA_LAUNCH(apgd_update_kernel<false>, grid, dim3(TPB), 0, x, x_old, x0, g, eta, plane, a, e, lo,
             hi, nonfinite);
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
  // every pair of the six arrays: fstate 4·N floats, istate 3·N ints, the others N words
  const float* b[6] = {loss, fstate, (const float*)istate, (const float*)action, hist_loss,
                       hist_eta};
  const int64_t len[6] = {N, 4LL * N, 3LL * N, N, N, N};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)  // b[j] must not start inside b[i]
      MIA_CHECK_ARG(i == j || b[j] < b[i] ||
                        (uintptr_t)b[j] - (uintptr_t)b[i] >= (uintptr_t)len[i] * sizeof(float),
                    "the state, action, loss and history arrays must be distinct buffers");
  MIA_LAUNCH(apgd_decide_kernel, dim3((N + 63) / 64), dim3(64), 0, loss, fstate, istate, action,
             hist_loss, hist_eta, N, step, checkpoint, thr, eta0);
}

extern "C" int mia_apgd_apply(float* x, float* g, float* x_best, float* g_best, const int* action,
                              int N, int64_t plane, void* stream) {
  MIA_CHECK_ARG(x && g && x_best && g_best && action, "null argument");
  MIA_CHECK_IMAGES(N, plane);
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(x, g, len) && !di_overlap(x, x_best, len) &&
                    !di_overlap(x, g_best, len) && !di_overlap(g, x_best, len) &&
                    !di_overlap(g, g_best, len) && !di_overlap(x_best, g_best, len),
                "x, g, x_best and g_best must be distinct buffers");
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(g) && aligned16(x_best) &&
                   aligned16(g_best);
  const dim3 grid = image_grid(plane + 3, 4, N);
  if (vec)
    MIA_LAUNCH(apgd_apply_kernel<true>, grid, dim3(TPB), 0, x, g, x_best, g_best, action, plane);
  MIA_LAUNCH(apgd_apply_kernel<false>, grid, dim3(TPB), 0, x, g, x_best, g_best, action, plane);
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
  MIA_CHECK_ARG(!di_overlap(x, x0, len) && !byte_overlap(x, len * 4, s, len) &&
                    !byte_overlap(x0, len * 4, s, len) &&
                    !(accept && (byte_overlap(accept, (int64_t)N * 4, x, len * 4) ||
                                 byte_overlap(accept, (int64_t)N * 4, x0, len * 4) ||
                                 byte_overlap(accept, (int64_t)N * 4, s, len))),
                "x, x0, s and accept must be distinct buffers");
  // the hull of the non-empty ranges, in groups of 4 elements counted from the image start
  const bool hp = prev_lo < prev_hi, hn = lo < hi;
  const int64_t h0 = hp && hn ? (prev_lo < lo ? prev_lo : lo) : hp ? prev_lo : lo;
  const int64_t h1 = hp && hn ? (prev_hi > hi ? prev_hi : hi) : hp ? prev_hi : hi;
  const int64_t g0 = h0 / 4, ng = (h1 + 3) / 4 - g0;
  const bool vec = plane % 4 == 0 && aligned16(x) && aligned16(x0) && ((uintptr_t)s & 3) == 0;
  const dim3 grid(blocks_for(ng, TPB, 1024), N);
  if (vec)
    MIA_LAUNCH(sh_flip_kernel<true>, grid, dim3(TPB), 0, x, x0, (signed char*)s, accept, plane, g0,
               ng, prev_lo, prev_hi, lo, hi, e, lo_v, hi_v);
  MIA_LAUNCH(sh_flip_kernel<false>, grid, dim3(TPB), 0, x, x0, (signed char*)s, accept, plane, g0,
             ng, prev_lo, prev_hi, lo, hi, e, lo_v, hi_v);
}

extern "C" int mia_sh_decide(const float* loss, float* best, int* accept, int* n_accept,
                             float* hist_loss, int N, int first, int* nonfinite, void* stream) {
  MIA_CHECK_ARG(loss && best && accept && n_accept && hist_loss, "null argument");
  MIA_CHECK_ARG(N > 0 && N <= 65535, "N must be in 1 … 65535");
  MIA_CHECK_ARG(first == 0 || first == 1, "first must be 0 or 1");
  // every pair of the arrays, N 4-byte words each
  const void* b[6] = {loss, best, accept, n_accept, hist_loss, nonfinite};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      MIA_CHECK_ARG(!b[i] || !b[j] || !byte_overlap(b[i], (int64_t)N * 4, b[j], (int64_t)N * 4),
                    "loss, best, accept, n_accept, hist_loss and nonfinite must be distinct buffers");
  MIA_LAUNCH(sh_decide_kernel, dim3((N + 63) / 64), dim3(64), 0, loss, best, accept, n_accept,
             hist_loss, N, first, nonfinite);
}

template <int K>
static int pi_launch(bool vec, dim3 grid, hipStream_t st, float* x, const float* x0, const float* g,
                     const float* l1, const float* m_in, float* m_out, const float* A_in,
                     float* A_out, int C, int H, int W, int tiles_x, int tiles_y, float mu, float ab,
                     float gm, float e, float lo, float hi, int* nonfinite) {
  if (vec)
    hipLaunchKernelGGL((pi_update_kernel<K, true>), grid, dim3(TPB), 0, st, x, x0, g, l1, m_in,
                       m_out, A_in, A_out, C, H, W, tiles_x, tiles_y, mu, ab, gm, e, lo, hi,
                       nonfinite);
  else
    hipLaunchKernelGGL((pi_update_kernel<K, false>), grid, dim3(TPB), 0, st, x, x0, g, l1, m_in,
                       m_out, A_in, A_out, C, H, W, tiles_x, tiles_y, mu, ab, gm, e, lo, hi,
                       nonfinite);
  return check_launch("pi_update_kernel");
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
  // buffer may overlap any other
  const int64_t len = (int64_t)N * plane;
  MIA_CHECK_ARG(!di_overlap(m_in, m_out, len), "m_in and m_out must be distinct buffers");
  MIA_CHECK_ARG(!di_overlap(A_in, A_out, len), "A_in and A_out must be distinct buffers");
  const float* wr[3] = {x, m_out, A_out};
  const float* rd[7] = {x0, g, m_in, A_in, x, m_out, A_out};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 7; ++j)
      MIA_CHECK_ARG(j == i + 4 || !di_overlap(wr[i], rd[j], len),
                    "x, x0, g, m_in, m_out, A_in and A_out must be distinct buffers");
  MIA_CHECK_ARG(!byte_overlap(l1, (int64_t)N * 4, x, len * 4) &&
                    !byte_overlap(l1, (int64_t)N * 4, m_out, len * 4) &&
                    !byte_overlap(l1, (int64_t)N * 4, A_out, len * 4),
                "l1 must not overlap x, m_out or A_out");
  const bool vec = W % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g) &&
                   aligned16(m_in) && aligned16(m_out) && aligned16(A_in) && aligned16(A_out);
  const int tiles_x = (W + TI_T - 1) / TI_T, tiles_y = (H + TI_T - 1) / TI_T;
  const dim3 grid(C * tiles_x * tiles_y, N);  // ≤ plane < 2^31 blocks per row
  const hipStream_t st = (hipStream_t)stream;
#define MIA_PI_CASE(k)                                                                          \
  case k:                                                                                       \
    return pi_launch<k>(vec, grid, st, x, x0, g, l1, m_in, m_out, A_in, A_out, C, H, W, tiles_x, \
                        tiles_y, mu, ab, gm, e, lo, hi, nonfinite)
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

extern "C" int mia_pixel_norm(const float* x, float* y, int rows, int cols, float eps,
                              void* stream) {
  MIA_CHECK_ARG(x && y && rows > 0 && cols > 0, "bad args");
  MIA_LAUNCH(pixel_norm_kernel, dim3(rows), dim3(TPB), 0, x, y, cols, eps);
}

extern "C" int mia_truncate(const float* w, const float* mean, float psi, float* out, int rows,
                            int cols, void* stream) {
  MIA_CHECK_ARG(w && mean && out && rows > 0 && cols > 0, "bad args");
  const int64_t len = (int64_t)rows * cols;
  MIA_LAUNCH(truncate_kernel, dim3(blocks_for(len, TPB, 65536)), dim3(TPB), 0, w, mean, psi, out,
             len, cols);
}

extern "C" int mia_repeat(const void* src, void* dst, int64_t bytes, int count, void* stream) {
  MIA_CHECK_ARG(src && dst && bytes > 0 && count > 0, "bad args");
  MIA_LAUNCH(repeat_kernel, dim3(blocks_for(bytes * count, TPB, 65536)), dim3(TPB), 0,
             (const uint8_t*)src, (uint8_t*)dst, bytes, count);
}

// Byte fill on the caller's stream as a kernel of our own (no hipMemsetAsync: the runtime's fill
// path crashed inside rocprofv3 --pmc collection, and a plain kernel is capturable like the rest):
// 16-byte stores when the buffer and length allow, else 4-byte, else bytes.
template <typename V>
__global__ void fill_kernel(V* __restrict__ dst, V v, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)mia::TPB + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * mia::TPB)
    dst[i] = v;
}

extern "C" int mia_memset(void* dst, int value, int64_t bytes, void* stream) {
  MIA_CHECK_ARG(dst && bytes >= 0, "bad args");
  if (bytes == 0) return MIA_OK;
  const unsigned b = (unsigned)value & 0xffu, w = b * 0x01010101u;
  const uintptr_t a = (uintptr_t)dst;
  if (a % 16 == 0 && bytes % 16 == 0) {
    const int64_t n = bytes / 16;
    MIA_LAUNCH(fill_kernel<uint4>, dim3(blocks_for(n, mia::TPB, 65536)), dim3(mia::TPB), 0,
               (uint4*)dst, make_uint4(w, w, w, w), n);
  } else if (a % 4 == 0 && bytes % 4 == 0) {
    const int64_t n = bytes / 4;
    MIA_LAUNCH(fill_kernel<unsigned>, dim3(blocks_for(n, mia::TPB, 65536)), dim3(mia::TPB), 0,
               (unsigned*)dst, w, n);
  } else {
    MIA_LAUNCH(fill_kernel<unsigned char>, dim3(blocks_for(bytes, mia::TPB, 65536)),
               dim3(mia::TPB), 0, (unsigned char*)dst, (unsigned char)b, bytes);
  }
  return MIA_OK;
}
