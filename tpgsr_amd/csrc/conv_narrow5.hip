// Direct 5x5, pad 2, stride 1 convolution to 1 <= Cout <= 4 channels on an NHWC map, optional bias -- SRCNN's conv3 (reference model/srcnn.py:
// Conv2d(32, 3, 5, padding=2) on the HR grid).  On the matrix-core routes Cout = 3 is padded to a 64-wide tile.  Cin is a multiple of 4 up to
// 64, so the lane map of the 3x3 kernels (one lane per four input channels, weights in registers: csrc/conv_narrow.hip) would leave most of
// a wave idle and need 100 Cout weight registers per lane.  Here a lane owns OUTPUT elements and the weights are staged once per workgroup in
// LDS -- w [Cout][Cin][5][5] as PyTorch stores it, regrouped while it is staged so that the four channels of a group are one 16-byte read:
//
//   tpgsr_conv5x5_narrow_fwd         a lane owns two neighbouring pixels of a row: per input row and channel group six 16-byte loads of x
//                                    feed 2 x 5 x 4 Cout multiply-adds; the weights come from LDS at wave-uniform addresses (a broadcast)
//   tpgsr_conv5x5_narrow_bwd_data    a gather: a lane owns eight channels of one pixel of dx, reads the 25 Cout dy values of its window and
//                                    the weights [tap][co][channel group] from LDS; two 16-byte stores per lane
//   tpgsr_conv5x5_narrow_bwd_weight  a workgroup sums its range of pixels in order; a thread owns one tap and one group of four channels
//                                    (4 Cout accumulators; the wave's loads of x are the contiguous channels of neighbouring pixels, dy is read
//                                    at wave-uniform addresses); [nblk][Cout Cin 25 + Cout] partial sums -- the weight elements in w's order,
//                                    then the bias gradient -- finished by tpgsr_reduce_partials
// Plain fp32 fused multiply-adds in a fixed order: no atomics, bitwise reproducible, independent of the arithmetic policy.  x and dx move in
// 16-byte accesses where the pointers are 16-byte aligned, element by element (the same bits) otherwise.
#include "common.h"

namespace {

constexpr int kMaxCout = 4;
constexpr int kMaxCin = 64;
constexpr int kMaxCin4 = kMaxCin / 4;
constexpr int kTaps = 25;
constexpr int kThreads = 256;
constexpr int kPix = 2;           // output pixels of one row per lane (forward)
constexpr int kChunk4 = 2;        // channel groups of four per lane (data gradient)

__device__ __forceinline__ float4 ld4(const float* p, int vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void st4(float* p, float4 v, int vec) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = __builtin_fmaf(a.x, b.x, acc);
  acc = __builtin_fmaf(a.y, b.y, acc);
  acc = __builtin_fmaf(a.z, b.z, acc);
  return __builtin_fmaf(a.w, b.w, acc);
}

// the four channels 4 c4 .. 4 c4 + 3 of tap t of output channel co
__device__ __forceinline__ float4 weight_group(const float* __restrict__ w, int Cin, int co, int c4, int t) {
  const float* p = w + ((size_t)co * Cin + 4 * c4) * kTaps + t;
  return make_float4(p[0], p[kTaps], p[2 * kTaps], p[3 * kTaps]);
}

template <int CO>
__global__ __launch_bounds__(kThreads) void narrow5_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                               int N, int H, int W, int Cin, int vec, float* __restrict__ y) {
  __shared__ float4 wl[kTaps * kMaxCin4 * CO];      // [tap][channel group][co]
  const int Cin4 = Cin >> 2;
  for (int i = threadIdx.x; i < kTaps * Cin4 * CO; i += kThreads) wl[i] = weight_group(w, Cin, i % CO, (i / CO) % Cin4, i / (CO * Cin4));
  __syncthreads();
  const int pairs = (W + kPix - 1) / kPix;
  const long long units = (long long)N * H * pairs;
  const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (u >= units) return;
  const long long nh = u / pairs;      // n * H + h
  const int q0 = (int)(u % pairs) * kPix, h = (int)(nh % H);
  float acc[kPix][CO];
#pragma unroll
  for (int k = 0; k < kPix; ++k)
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[k][co] = 0.f;
  // fixed order: the five input rows top down, the channel groups, the five taps of the row, the four channels of a group
  for (int r = 0; r < 5; ++r) {
    if ((unsigned)(h + r - 2) >= (unsigned)H) continue;
    const float* xrow = x + (size_t)(nh + r - 2) * W * Cin;
    for (int c4 = 0; c4 < Cin4; ++c4) {
      float4 xv[kPix + 4];
#pragma unroll
      for (int k = 0; k < kPix + 4; ++k) {
        const int q = q0 - 2 + k;
        xv[k] = (unsigned)q < (unsigned)W ? ld4(xrow + (size_t)q * Cin + 4 * c4, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int s = 0; s < 5; ++s)
#pragma unroll
        for (int co = 0; co < CO; ++co) {
          const float4 wv = wl[((r * 5 + s) * Cin4 + c4) * CO + co];
#pragma unroll
          for (int k = 0; k < kPix; ++k) acc[k][co] = dot4(xv[s + k], wv, acc[k][co]);
        }
    }
  }
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    if (q0 + k >= W) break;
    float* out = y + ((size_t)nh * W + q0 + k) * CO;
#pragma unroll
    for (int co = 0; co < CO; ++co) out[co] = bias ? acc[k][co] + bias[co] : acc[k][co];
  }
}

// dx[n][h][q][ci] = sum_r sum_s sum_co dy[n][h - r + 2][q - s + 2][co] * w[co][ci][r][s]
template <int CO>
__global__ __launch_bounds__(kThreads) void narrow5_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int H, int W,
                                                                    int Cin, int vec, float* __restrict__ dx) {
  __shared__ float4 wl[kTaps * CO * kMaxCin4];      // [tap][co][channel group]
  const int Cin4 = Cin >> 2;
  for (int i = threadIdx.x; i < kTaps * CO * Cin4; i += kThreads) wl[i] = weight_group(w, Cin, (i / Cin4) % CO, i % Cin4, i / (Cin4 * CO));
  __syncthreads();
  const int chunks = (Cin4 + kChunk4 - 1) / kChunk4;
  const long long units = (long long)N * H * W * chunks;
  const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (u >= units) return;
  const long long p = u / chunks, nh = p / W;
  const int ca = (int)(u % chunks) * kChunk4, q = (int)(p % W), h = (int)(nh % H);
  const bool two = ca + 1 < Cin4;
  const int cb = two ? ca + 1 : ca;                 // (a lane past the last group computes group ca twice and stores it once)
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  // fixed order: the taps row by row, the output channels inside a tap
  for (int r = 0; r < 5; ++r) {
    if ((unsigned)(h - r + 2) >= (unsigned)H) continue;
    for (int s = 0; s < 5; ++s) {
      const int ow = q - s + 2;
      if ((unsigned)ow >= (unsigned)W) continue;
      const float* g = dy + ((size_t)(nh - r + 2) * W + ow) * CO;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float gv = g[co];
        const float4 wa = wl[((r * 5 + s) * CO + co) * Cin4 + ca], wb = wl[((r * 5 + s) * CO + co) * Cin4 + cb];
        a.x = __builtin_fmaf(gv, wa.x, a.x); a.y = __builtin_fmaf(gv, wa.y, a.y);
        a.z = __builtin_fmaf(gv, wa.z, a.z); a.w = __builtin_fmaf(gv, wa.w, a.w);
        b.x = __builtin_fmaf(gv, wb.x, b.x); b.y = __builtin_fmaf(gv, wb.y, b.y);
        b.z = __builtin_fmaf(gv, wb.z, b.z); b.w = __builtin_fmaf(gv, wb.w, b.w);
      }
    }
  }
  float* out = dx + (size_t)p * Cin;
  st4(out + 4 * ca, a, vec);
  if (two) st4(out + 4 * cb, b, vec);
}

// partial[blk][(co * Cin + ci) * 25 + t]: sum over the workgroup's pixels [blk * per_blk, (blk + 1) * per_blk) in order of
// x[n][h + r - 2][q + s - 2][ci] * dy[n][h][q][co]; partial[blk][Cout Cin 25 + co]: the sum of dy[..][co] over the same pixels
template <int CO>
__global__ __launch_bounds__(kThreads) void narrow5_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int H, int W,
                                                                      int Cin, int vec, long long per_blk, float* __restrict__ partial) {
  const int Cin4 = Cin >> 2;
  const long long M = (long long)N * H * W;
  const long long p0 = min(M, (long long)blockIdx.x * per_blk), p1 = min(M, p0 + per_blk);
  const size_t E = (size_t)CO * Cin * kTaps;
  float* row = partial + (size_t)blockIdx.x * (E + CO);      // (workgroups past the last pixel write zeros: every row is defined)
  const long long nh0 = p0 / W;
  const int q0 = (int)(p0 % W), h0 = (int)(nh0 % H);
  for (int item = threadIdx.x; item < kTaps * Cin4; item += kThreads) {
    const int t = item / Cin4, c4 = item % Cin4, r = t / 5, s = t % 5;
    float acc[CO][4];
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[co][k] = 0.f;
    long long nh = nh0;
    int q = q0, h = h0;
#pragma unroll 4
    for (long long p = p0; p < p1; ++p) {
      const int iq = q + s - 2;
      const bool in = (unsigned)(h + r - 2) < (unsigned)H && (unsigned)iq < (unsigned)W;
      const float4 xv = in ? ld4(x + ((size_t)(nh + r - 2) * W + iq) * Cin + 4 * c4, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float* g = dy + (size_t)p * CO;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float gv = g[co];
        acc[co][0] = __builtin_fmaf(xv.x, gv, acc[co][0]);
        acc[co][1] = __builtin_fmaf(xv.y, gv, acc[co][1]);
        acc[co][2] = __builtin_fmaf(xv.z, gv, acc[co][2]);
        acc[co][3] = __builtin_fmaf(xv.w, gv, acc[co][3]);
      }
      if (++q == W) {
        q = 0;
        ++nh;
        if (++h == H) h = 0;
      }
    }
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
      for (int k = 0; k < 4; ++k) row[((size_t)co * Cin + 4 * c4 + k) * kTaps + t] = acc[co][k];
  }
  if (threadIdx.x < CO) {
    float sum = 0.f;
    for (long long p = p0; p < p1; ++p) sum += dy[(size_t)p * CO + threadIdx.x];
    row[E + threadIdx.x] = sum;
  }
}

bool narrow5_args_ok(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout < 1 || Cout > kMaxCout || Cin < 4 || Cin > kMaxCin || (Cin & 3)) return false;
  return (long long)N * H * W < (1ll << 27);
}

#define NARROW5_ARGS_MSG \
  ": takes 1 <= Cout <= 4, Cin a multiple of 4 up to 64 and fewer than 2^27 pixels (got N %d, H %d, W %d, Cin %d, Cout %d)"

inline int blocks_for(long long units) { return (int)((units + kThreads - 1) / kThreads); }

inline int aligned16(const void* a) { return (((uintptr_t)a) & 15) == 0; }

}  // namespace

#define NARROW5_DISPATCH(kernel, grid, ...)                                                                          \
  switch (Cout) {                                                                                                    \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(kThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(kThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL(kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;        \
  }

extern "C" int tpgsr_conv5x5_narrow_fwd(const float* x, const float* w, const float* bias, int N, int H, int W, int Cin, int Cout, float* y,
                                        void* stream) {
  TPGSR_CHECK_ARG(x && w && y, "tpgsr_conv5x5_narrow_fwd: null pointer");
  TPGSR_CHECK_ARG(narrow5_args_ok(N, H, W, Cin, Cout), "tpgsr_conv5x5_narrow_fwd" NARROW5_ARGS_MSG, N, H, W, Cin, Cout);
  const long long units = (long long)N * H * ((W + kPix - 1) / kPix);
  NARROW5_DISPATCH(narrow5_fwd_kernel, dim3(blocks_for(units)), x, w, bias, N, H, W, Cin, aligned16(x), y);
  TPGSR_LAUNCH_CHECK("tpgsr_conv5x5_narrow_fwd");
}

extern "C" int tpgsr_conv5x5_narrow_bwd_data(const float* dy, const float* w, int N, int H, int W, int Cin, int Cout, float* dx, void* stream) {
  TPGSR_CHECK_ARG(dy && w && dx, "tpgsr_conv5x5_narrow_bwd_data: null pointer");
  TPGSR_CHECK_ARG(narrow5_args_ok(N, H, W, Cin, Cout), "tpgsr_conv5x5_narrow_bwd_data" NARROW5_ARGS_MSG, N, H, W, Cin, Cout);
  const long long units = (long long)N * H * W * (((Cin >> 2) + kChunk4 - 1) / kChunk4);
  NARROW5_DISPATCH(narrow5_bwd_data_kernel, dim3(blocks_for(units)), dy, w, N, H, W, Cin, aligned16(dx), dx);
  TPGSR_LAUNCH_CHECK("tpgsr_conv5x5_narrow_bwd_data");
}

extern "C" int tpgsr_conv5x5_narrow_bwd_weight(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout, float* partial, int nblk,
                                               void* stream) {
  TPGSR_CHECK_ARG(x && dy && partial && nblk > 0 && nblk <= 65536, "tpgsr_conv5x5_narrow_bwd_weight: bad arguments (1 <= nblk <= 65536)");
  TPGSR_CHECK_ARG(narrow5_args_ok(N, H, W, Cin, Cout), "tpgsr_conv5x5_narrow_bwd_weight" NARROW5_ARGS_MSG, N, H, W, Cin, Cout);
  const long long M = (long long)N * H * W;
  const long long per_blk = (M + nblk - 1) / nblk;
  NARROW5_DISPATCH(narrow5_bwd_weight_kernel, dim3(nblk), x, dy, N, H, W, Cin, aligned16(x), per_blk, partial);
  TPGSR_LAUNCH_CHECK("tpgsr_conv5x5_narrow_bwd_weight");
}
