// What the translation units of the attack-step kernels (attack_step.hip, jpeg.hip) share: the
// 16-byte / scalar accessors, the per-image partial-sum store of the *_norms kernels, and the
// launchers' helpers (the vec decision, the two-instantiation launch, the ordered-norms launch and
// the buffer-overlap checks).
#pragma once
#include <initializer_list>

#include "pointwise_common.h"

namespace mia {

// The *_norms kernels run on a (slots, N) grid, block (b, n) working on image n alone: an image's
// partial sums — and so its norms — depend on its own plane size only, never on the other images
// of the call. V = 4: 16-byte accesses (plane % 4 == 0 and 16-byte aligned bases, decided by the
// launcher); V = 1: scalar.
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

// ---- what the launchers share ------------------------------------------------------------------
// A launcher reads: argument checks, the vec decision, the grid, one launch statement.

// The 16-byte form of a kernel: n (the plane, or the row length of a tiled kernel) is a multiple
// of 4 and every base is 16-byte aligned. An absent (null) operand counts as aligned.
static inline bool vec_ok(int64_t n, std::initializer_list<const void*> bases) {
  bool ok = n % 4 == 0;
  for (const void* p : bases) ok = ok && ((uintptr_t)p & 15) == 0;
  return ok;
}

// The 16-byte (vec) or the scalar instantiation of a kernel, TPB threads per block, on ONE
// argument list; `what` names the kernel in a launch error.
template <typename... P, typename... A>
static int launch2(const char* what, void (*kvec)(P...), void (*kscalar)(P...), bool vec, dim3 grid,
                   size_t lds, hipStream_t st, A... args) {
  hipLaunchKernelGGL(vec ? kvec : kscalar, grid, dim3(TPB), lds, st, args...);
  return check_launch(what);
}

// A launch whose blocks store per-image partial sums of up to two quantities: red_begin (grid.x
// slots for each of N images), launch(part) — the launcher puts the partial buffer where its
// kernel takes it — and red_finish, which adds the slots in order into d0 / d1 (null: absent).
template <typename F>
static int launch_norms(float* d0, float* d1, dim3 grid, int N, hipStream_t st, F launch) {
  RedQ r;
  int rc = red_begin(r, d0, d1, nullptr, grid.x, N, st);
  if (rc != MIA_OK) return rc;
  rc = launch(r.part);
  return rc != MIA_OK ? rc : red_finish(r, st);
}

// A buffer argument as (base, byte length); words(): n floats or ints.
struct Span {
  const void* p;
  int64_t bytes;
};
static inline Span words(const void* p, int64_t n) { return {p, n * 4}; }

static inline bool overlap(Span a, Span b) {
  const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
  return pa < pb ? pb - pa < (uintptr_t)a.bytes : pa - pb < (uintptr_t)b.bytes;
}

// no two of these buffers overlap; absent (null) ones are skipped
static inline bool disjoint(std::initializer_list<Span> s) {
  for (const Span* a = s.begin(); a != s.end(); ++a)
    for (const Span* b = a + 1; b != s.end(); ++b)
      if (a->p && b->p && overlap(*a, *b)) return false;
  return true;
}

}  // namespace mia

#define MIA_CHECK_IMAGES(N, plane)                                                      \
  MIA_CHECK_ARG((N) > 0 && (N) <= 65535, "N must be in 1 … 65535");                     \
  MIA_CHECK_ARG((plane) > 0 && (plane) < (1LL << 31), "plane must be in 1 … 2^31 − 1")
