// Glue of the in-place residual dense block (functional.dense_block; reference model/esrgan.py:16-36 ResidualDenseBlock_5C): the block's
// five convolutions read and write channel windows of ONE concatenation buffer, and these three kernels are what is left between them.
//   tpgsr_leaky_relu_window   LeakyReLU in place on the window a convolution just wrote
//   tpgsr_scaled_add          out = alpha * a + b over windows (the 0.2-scaled residuals of the block and of RRDB)
//   tpgsr_dense_bwd_step      one pass of the in-place backward: accumulate a data gradient into the gradient buffer's prefix and mask
//                             the next window by the activation's derivative, or (last pass) write the block's input gradient
// Buffers are NHWC rows [M][ld]; a window is the channels [coff, coff + C) of every row.  HBM-bound, one pass each: 256-thread blocks, a
// grid-stride loop over at most 4096 blocks; 16-byte accesses when every pointer, row length and window bound is a multiple of 16 bytes,
// element by element otherwise.  No kernel touches a column outside its windows or a row at or behind M.  Pointers that may alias (in-place
// forms) are not __restrict__: every thread reads the elements it writes, nothing else.
#include "common.h"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// flat index -> (row, position in the window); a 32-bit division while the index space allows it
__device__ __forceinline__ void row_pos(long long i, int cw, bool small, long long& m, int& q) {
  if (small) {
    const unsigned u = (unsigned)i, r = u / (unsigned)cw;
    m = r;
    q = (int)(u - r * (unsigned)cw);
  } else {
    m = i / cw;
    q = (int)(i - m * cw);
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline int grid_for(long long work) { return (int)max((long long)1, min((long long)4096, (work + 255) / 256)); }

__device__ __forceinline__ float leaky(float x, float v, float slope) { return x > 0.f ? v : v * slope; }

// alpha * a + b as a rounded product followed by a rounded sum: contraction into one fused multiply-add is switched OFF for this
// function (hipcc contracts device code by default), so the result is the float32 expression's, operation by operation
__device__ __forceinline__ float mul_then_add(float alpha, float a, float b) {
#pragma clang fp contract(off)
  const float p = alpha * a;
  return p + b;
}

template <bool VEC>
__global__ __launch_bounds__(256) void leaky_relu_window_kernel(float* buf, int ld, int coff, int cw, long long total, bool small, float slope) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    long long m;
    int q;
    row_pos(i, cw, small, m, q);
    if (VEC) {
      float* p = buf + m * ld + coff + 4 * q;
      const float4 v = ld4(p);
      st4(p, make_float4(leaky(v.x, v.x, slope), leaky(v.y, v.y, slope), leaky(v.z, v.z, slope), leaky(v.w, v.w, slope)));
    } else {
      float* p = buf + m * ld + coff + q;
      const float v = *p;
      *p = leaky(v, v, slope);
    }
  }
}

template <bool VEC, bool HAS_B>
__global__ __launch_bounds__(256) void scaled_add_kernel(const float* a, int a_ld, int a_coff, const float* b, int b_ld, int b_coff, float alpha,
                                                         float* out, int out_ld, int out_coff, int cw, long long total, bool small) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    long long m;
    int q;
    row_pos(i, cw, small, m, q);
    if (VEC) {
      const float4 u = ld4(a + m * a_ld + a_coff + 4 * q);
      const float4 v = HAS_B ? ld4(b + m * b_ld + b_coff + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      st4(out + m * out_ld + out_coff + 4 * q,
          HAS_B ? make_float4(mul_then_add(alpha, u.x, v.x), mul_then_add(alpha, u.y, v.y), mul_then_add(alpha, u.z, v.z), mul_then_add(alpha, u.w, v.w))
                : make_float4(alpha * u.x, alpha * u.y, alpha * u.z, alpha * u.w));
    } else {
      const float u = a[m * a_ld + a_coff + q];
      out[m * out_ld + out_coff + q] = HAS_B ? mul_then_add(alpha, u, b[m * b_ld + b_coff + q]) : alpha * u;
    }
  }
}

// FINAL = false: G[m][c0 + c] (+= T[m][c0 + c] when T) and, inside the mask window, *= (D > 0 ? 1 : slope); the loop covers [c0, c0 + cw)
//                (c0 = 0 with T, the mask window alone without).  FINAL: dx[m][c] = (G[m][c] + T[m][c]) + skip[m][c], G untouched.
template <bool VEC, bool FINAL>
__global__ __launch_bounds__(256) void dense_bwd_step_kernel(float* G, int ld, const float* T, int c_acc, const float* D, int c0, int cw, int mask_lo,
                                                             int mask_hi, float slope, const float* skip, float* dx, long long total, bool small) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    long long m;
    int q;
    row_pos(i, cw, small, m, q);
    if (VEC) {
      const int c = c0 + 4 * q;
      float4 g = ld4(G + m * ld + c);
      if (T) {
        const float4 t = ld4(T + m * c_acc + c);
        g.x += t.x; g.y += t.y; g.z += t.z; g.w += t.w;
      }
      if (FINAL) {
        if (skip) {
          const float4 s = ld4(skip + m * c_acc + c);
          g.x += s.x; g.y += s.y; g.z += s.z; g.w += s.w;
        }
        st4(dx + m * c_acc + c, g);
      } else {
        if (c >= mask_lo && c < mask_hi) {      // (window bounds are multiples of 4 on this path: a group is inside or outside as a whole)
          const float4 d = ld4(D + m * ld + c);
          g = make_float4(leaky(d.x, g.x, slope), leaky(d.y, g.y, slope), leaky(d.z, g.z, slope), leaky(d.w, g.w, slope));
        }
        st4(G + m * ld + c, g);
      }
    } else {
      const int c = c0 + q;
      float g = G[m * ld + c];
      if (T) g += T[m * c_acc + c];
      if (FINAL) {
        if (skip) g += skip[m * c_acc + c];
        dx[m * c_acc + c] = g;
      } else {
        if (c >= mask_lo && c < mask_hi) g = leaky(D[m * ld + c], g, slope);
        G[m * ld + c] = g;
      }
    }
  }
}

}  // namespace

extern "C" int tpgsr_leaky_relu_window(float* buf, int ld, int coff, int C, long long M, float slope, void* stream) {
  TPGSR_CHECK_ARG(buf && M > 0 && C > 0 && coff >= 0 && ld >= coff + C, "tpgsr_leaky_relu_window: bad arguments");
  const bool vec = aligned16(buf) && ((ld | coff | C) & 3) == 0;
  const int cw = vec ? C / 4 : C;
  const long long total = M * cw;
  const bool small = total <= 0x7fffffffLL;
  if (vec)
    hipLaunchKernelGGL(leaky_relu_window_kernel<true>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, buf, ld, coff, cw, total, small, slope);
  else
    hipLaunchKernelGGL(leaky_relu_window_kernel<false>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, buf, ld, coff, cw, total, small, slope);
  TPGSR_LAUNCH_CHECK("tpgsr_leaky_relu_window");
}

extern "C" int tpgsr_scaled_add(const float* a, int a_ld, int a_coff, const float* b, int b_ld, int b_coff, float alpha, float* out, int out_ld,
                                int out_coff, long long M, int C, void* stream) {
  TPGSR_CHECK_ARG(a && out && M > 0 && C > 0 && a_coff >= 0 && a_ld >= a_coff + C && out_coff >= 0 && out_ld >= out_coff + C &&
                      (!b || (b_coff >= 0 && b_ld >= b_coff + C)),
                  "tpgsr_scaled_add: bad arguments");
  const bool vec = aligned16(a) && aligned16(b) && aligned16(out) && ((a_ld | a_coff | out_ld | out_coff | C) & 3) == 0 && (!b || ((b_ld | b_coff) & 3) == 0);
  const int cw = vec ? C / 4 : C;
  const long long total = M * cw;
  const bool small = total <= 0x7fffffffLL;
  const dim3 grid(grid_for(total)), block(256);
#define TPGSR_SA(V, B) \
  hipLaunchKernelGGL((scaled_add_kernel<V, B>), grid, block, 0, (hipStream_t)stream, a, a_ld, a_coff, b, b_ld, b_coff, alpha, out, out_ld, out_coff, cw, total, small)
  if (vec && b) TPGSR_SA(true, true);
  else if (vec) TPGSR_SA(true, false);
  else if (b) TPGSR_SA(false, true);
  else TPGSR_SA(false, false);
#undef TPGSR_SA
  TPGSR_LAUNCH_CHECK("tpgsr_scaled_add");
}

extern "C" int tpgsr_dense_bwd_step(float* G, int ld, const float* T, int c_acc, const float* Dbuf, int mask_coff, int mask_c, float slope,
                                    const float* skip, float* dx, long long M, void* stream) {
  TPGSR_CHECK_ARG(G && M > 0 && c_acc > 0 && ld >= c_acc && mask_coff >= 0 && mask_c >= 0 && mask_coff + mask_c <= c_acc && (mask_c == 0 || Dbuf) &&
                      (dx ? (T && mask_c == 0) : (!skip && (T || mask_c > 0))),
                  "tpgsr_dense_bwd_step: bad arguments");
  const int c0 = T ? 0 : mask_coff, cn = T ? c_acc : mask_c;      // without T there is nothing to add outside the mask window
  const bool vec = aligned16(G) && aligned16(T) && aligned16(Dbuf) && aligned16(skip) && aligned16(dx) && ((ld | c_acc | mask_coff | mask_c) & 3) == 0;
  const int cw = vec ? cn / 4 : cn;
  const long long total = M * cw;
  const bool small = total <= 0x7fffffffLL;
  const dim3 grid(grid_for(total)), block(256);
#define TPGSR_DB(V, F) \
  hipLaunchKernelGGL((dense_bwd_step_kernel<V, F>), grid, block, 0, (hipStream_t)stream, G, ld, T, c_acc, Dbuf, c0, cw, mask_coff, mask_coff + mask_c, slope, skip, dx, total, small)
  if (vec && dx) TPGSR_DB(true, true);
  else if (vec) TPGSR_DB(true, false);
  else if (dx) TPGSR_DB(false, true);
  else TPGSR_DB(false, false);
#undef TPGSR_DB
  TPGSR_LAUNCH_CHECK("tpgsr_dense_bwd_step");
}
