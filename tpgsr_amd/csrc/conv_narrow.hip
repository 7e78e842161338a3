// Direct 3x3, pad 1, stride 1 convolution to 1 <= Cout <= 4 channels on an NHWC map, no bias -- EDSR's conv_output (reference model/edsr.py:57:
// 256 -> 3 on the HR grid).  On the matrix-core routes Cout = 3 is padded to a 64-wide tile; here every lane of a wave owns FOUR input
// channels (one 16-byte load per pixel; Cin <= 256, a multiple of 4) together with its 4 x 9 x Cout weights -- w [Cout][Cin][3][3] as PyTorch
// stores it: the 36 floats of a lane's four channels are contiguous per output channel -- which stay in registers for the whole launch:
//
//   tpgsr_conv3x3_narrow_fwd         a wave walks a run of <= 32 output pixels of one row; its 3 x 3 window of 16-byte loads slides (three new
//                                    loads per pixel: each input row of the run is fetched once, not once per tap); 36 Cout multiply-adds
//                                    per lane, then a butterfly sum over the wave
//   tpgsr_conv3x3_narrow_bwd_data    a gather: dx[p][ci] from the 27 dy values of the 3 x 3 neighbourhood (wave-uniform loads), one 16-byte
//                                    store per lane and pixel -- bound by writing dx
//   tpgsr_conv3x3_narrow_bwd_weight  one single-wave workgroup per range of runs, a lane accumulates its 36 Cout weight elements over the
//                                    range in order; [nblk][Cout Cin 9] partial sums, finished by tpgsr_reduce_partials
// Plain fp32 fused multiply-adds in a fixed order: no atomics, bitwise reproducible, independent of the arithmetic policy.
#include "common.h"

namespace {

constexpr int kMaxCout = 4;
constexpr int kMaxCin = 256;      // 64 lanes x 4 channels
constexpr int kRun = 32;          // output pixels of one row per run
constexpr int kWaves = 4;         // runs a 256-thread workgroup works on at a time (forward, data gradient)
constexpr int kGridCap = 2048;    // grid-stride the rest

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

// wr[co][c * 9 + t] = w[co][c0 + c][t] for the lane's channels c0 .. c0 + 3 (zeros for a lane past Cin)
template <int CO>
__device__ __forceinline__ void load_weights(const float* __restrict__ w, int Cin, int c0, bool live, int vec, float (&wr)[CO][36]) {
#pragma unroll
  for (int co = 0; co < CO; ++co)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float4 v = live ? ld4(w + ((size_t)co * Cin + c0) * 9 + 4 * k, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
      wr[co][4 * k] = v.x; wr[co][4 * k + 1] = v.y; wr[co][4 * k + 2] = v.z; wr[co][4 * k + 3] = v.w;
    }
}

// the lane's four channels of pixel (row nh + d - 1, column q) of x, zeros outside the image (nh = n * H + h: the row above / below row h of
// the same image is row nh -+ 1 wherever it exists)
__device__ __forceinline__ float4 load_px(const float* __restrict__ x, long long nh, int h, int d, int q, int H, int W, int Cin, int c0, bool live,
                                          int vec) {
  if (!live || (unsigned)(h + d - 1) >= (unsigned)H || (unsigned)q >= (unsigned)W) return make_float4(0.f, 0.f, 0.f, 0.f);
  return ld4(x + ((size_t)(nh + d - 1) * W + q) * Cin + c0, vec);
}

struct Run {
  long long nh;      // n * H + h
  int h, w0, w1;
};

__device__ __forceinline__ Run run_of(long long r, int segs, int H, int W) {
  Run u;
  u.nh = r / segs;
  u.h = (int)(u.nh % H);
  u.w0 = (int)(r % segs) * kRun;
  u.w1 = min(W, u.w0 + kRun);
  return u;
}

template <int CO>
__global__ __launch_bounds__(64 * kWaves) void narrow_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int H, int W, int Cin,
                                                                 int vec, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, c0 = lane * 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = c0 < Cin;
  float wr[CO][36];
  load_weights<CO>(w, Cin, c0, live, vec, wr);
  const int segs = (W + kRun - 1) / kRun;
  const long long runs = (long long)N * H * segs;
  for (long long r = (long long)blockIdx.x * kWaves + wave; r < runs; r += (long long)gridDim.x * kWaves) {
    const Run u = run_of(r, segs, H, W);
    float4 win[3][3];      // [row h - 1 .. h + 1][column q - 1 .. q + 1]
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      win[d][1] = load_px(x, u.nh, u.h, d, u.w0 - 1, H, W, Cin, c0, live, vec);
      win[d][2] = load_px(x, u.nh, u.h, d, u.w0, H, W, Cin, c0, live, vec);
    }
    for (int q = u.w0; q < u.w1; ++q) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        win[d][0] = win[d][1];
        win[d][1] = win[d][2];
        win[d][2] = load_px(x, u.nh, u.h, d, q + 1, H, W, Cin, c0, live, vec);
      }
      float acc[CO];
#pragma unroll
      for (int co = 0; co < CO; ++co) acc[co] = 0.f;
      // fixed order: the nine taps row by row, the lane's four channels inside a tap; then the butterfly over the wave
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int t = d * 3 + s;
          const float4 xv = win[d][s];
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            acc[co] = __builtin_fmaf(xv.x, wr[co][t], acc[co]);
            acc[co] = __builtin_fmaf(xv.y, wr[co][9 + t], acc[co]);
            acc[co] = __builtin_fmaf(xv.z, wr[co][18 + t], acc[co]);
            acc[co] = __builtin_fmaf(xv.w, wr[co][27 + t], acc[co]);
          }
        }
      float mine = 0.f;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float v = wave_sum(acc[co]);
        if (lane == co) mine = v;
      }
      if (lane < CO) y[((size_t)u.nh * W + q) * CO + lane] = mine;
    }
  }
}

// dx[n][h][q][ci] = sum_r sum_s sum_co dy[n][h - r + 1][q - s + 1][co] * w[co][ci][r][s]
template <int CO>
__global__ __launch_bounds__(64 * kWaves) void narrow_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int H, int W,
                                                                      int Cin, int vec, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63, c0 = lane * 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = c0 < Cin;
  float wr[CO][36];
  load_weights<CO>(w, Cin, c0, live, vec, wr);
  const int segs = (W + kRun - 1) / kRun;
  const long long runs = (long long)N * H * segs;
  for (long long r = (long long)blockIdx.x * kWaves + wave; r < runs; r += (long long)gridDim.x * kWaves) {
    const Run u = run_of(r, segs, H, W);
    for (int q = u.w0; q < u.w1; ++q) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int rr = 0; rr < 3; ++rr) {
        const int oh = u.h - rr + 1;
        if ((unsigned)oh >= (unsigned)H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int ow = q - s + 1;
          if ((unsigned)ow >= (unsigned)W) continue;
          const int t = rr * 3 + s;
          const float* g = dy + ((size_t)(u.nh - rr + 1) * W + ow) * CO;
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            const float gv = g[co];
            acc.x = __builtin_fmaf(gv, wr[co][t], acc.x);
            acc.y = __builtin_fmaf(gv, wr[co][9 + t], acc.y);
            acc.z = __builtin_fmaf(gv, wr[co][18 + t], acc.z);
            acc.w = __builtin_fmaf(gv, wr[co][27 + t], acc.w);
          }
        }
      }
      if (live) st4(dx + ((size_t)u.nh * W + q) * Cin + c0, acc, vec);
    }
  }
}

// partial[blk][(co * Cin + ci) * 9 + t]: sum over the workgroup's runs [blk * per_blk, (blk + 1) * per_blk), pixel by pixel in order, of
// x[n][h + r - 1][q + s - 1][ci] * dy[n][h][q][co]
template <int CO>
__global__ __launch_bounds__(64) void narrow_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int H, int W, int Cin,
                                                               int vec, long long per_blk, float* __restrict__ partial) {
  const int lane = threadIdx.x, c0 = lane * 4;
  const bool live = c0 < Cin;
  float acc[CO][36];
#pragma unroll
  for (int co = 0; co < CO; ++co)
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[co][k] = 0.f;
  const int segs = (W + kRun - 1) / kRun;
  const long long runs = (long long)N * H * segs;
  const long long r0 = (long long)blockIdx.x * per_blk, r1 = min(runs, r0 + per_blk);
  for (long long r = r0; r < r1; ++r) {
    const Run u = run_of(r, segs, H, W);
    float4 win[3][3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      win[d][1] = load_px(x, u.nh, u.h, d, u.w0 - 1, H, W, Cin, c0, live, vec);
      win[d][2] = load_px(x, u.nh, u.h, d, u.w0, H, W, Cin, c0, live, vec);
    }
    for (int q = u.w0; q < u.w1; ++q) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        win[d][0] = win[d][1];
        win[d][1] = win[d][2];
        win[d][2] = load_px(x, u.nh, u.h, d, q + 1, H, W, Cin, c0, live, vec);
      }
      const float* g = dy + ((size_t)u.nh * W + q) * CO;
#pragma unroll
      for (int co = 0; co < CO; ++co) {
        const float gv = g[co];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            const int t = d * 3 + s;
            const float4 xv = win[d][s];
            acc[co][t] = __builtin_fmaf(xv.x, gv, acc[co][t]);
            acc[co][9 + t] = __builtin_fmaf(xv.y, gv, acc[co][9 + t]);
            acc[co][18 + t] = __builtin_fmaf(xv.z, gv, acc[co][18 + t]);
            acc[co][27 + t] = __builtin_fmaf(xv.w, gv, acc[co][27 + t]);
          }
      }
    }
  }
  if (!live) return;
  float* row = partial + (size_t)blockIdx.x * ((size_t)CO * Cin * 9);      // (workgroups past the last run write zeros: every row is defined)
#pragma unroll
  for (int co = 0; co < CO; ++co)
#pragma unroll
    for (int k = 0; k < 9; ++k)
      st4(row + ((size_t)co * Cin + c0) * 9 + 4 * k, make_float4(acc[co][4 * k], acc[co][4 * k + 1], acc[co][4 * k + 2], acc[co][4 * k + 3]), vec);
}

bool narrow_args_ok(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout < 1 || Cout > kMaxCout || Cin < 4 || Cin > kMaxCin || (Cin & 3)) return false;
  return (long long)N * H * W < (1ll << 27);
}

#define NARROW_ARGS_MSG \
  ": takes 1 <= Cout <= 4, Cin a multiple of 4 up to 256 and fewer than 2^27 pixels (got N %d, H %d, W %d, Cin %d, Cout %d)"

int capped_grid(long long runs) { return (int)max((long long)1, min((long long)kGridCap, (runs + kWaves - 1) / kWaves)); }

long long run_count(int N, int H, int W) { return (long long)N * H * ((W + kRun - 1) / kRun); }

inline int aligned16(const void* a, const void* b, const void* c) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) == 0; }

}  // namespace

#define NARROW_DISPATCH(kernel, grid, block, ...)                                                              \
  switch (Cout) {                                                                                              \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;            \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;            \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;            \
    default: hipLaunchKernelGGL(kernel<4>, grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;           \
  }

extern "C" int tpgsr_conv3x3_narrow_fwd(const float* x, const float* w, int N, int H, int W, int Cin, int Cout, float* y, void* stream) {
  TPGSR_CHECK_ARG(x && w && y, "tpgsr_conv3x3_narrow_fwd: null pointer");
  TPGSR_CHECK_ARG(narrow_args_ok(N, H, W, Cin, Cout), "tpgsr_conv3x3_narrow_fwd" NARROW_ARGS_MSG, N, H, W, Cin, Cout);
  const int vec = aligned16(x, w, nullptr);
  NARROW_DISPATCH(narrow_fwd_kernel, dim3(capped_grid(run_count(N, H, W))), dim3(64 * kWaves), x, w, N, H, W, Cin, vec, y);
  TPGSR_LAUNCH_CHECK("tpgsr_conv3x3_narrow_fwd");
}

extern "C" int tpgsr_conv3x3_narrow_bwd_data(const float* dy, const float* w, int N, int H, int W, int Cin, int Cout, float* dx, void* stream) {
  TPGSR_CHECK_ARG(dy && w && dx, "tpgsr_conv3x3_narrow_bwd_data: null pointer");
  TPGSR_CHECK_ARG(narrow_args_ok(N, H, W, Cin, Cout), "tpgsr_conv3x3_narrow_bwd_data" NARROW_ARGS_MSG, N, H, W, Cin, Cout);
  const int vec = aligned16(dx, w, nullptr);
  NARROW_DISPATCH(narrow_bwd_data_kernel, dim3(capped_grid(run_count(N, H, W))), dim3(64 * kWaves), dy, w, N, H, W, Cin, vec, dx);
  TPGSR_LAUNCH_CHECK("tpgsr_conv3x3_narrow_bwd_data");
}

extern "C" int tpgsr_conv3x3_narrow_bwd_weight(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout, float* partial, int nblk,
                                               void* stream) {
  TPGSR_CHECK_ARG(x && dy && partial && nblk > 0 && nblk <= 65536, "tpgsr_conv3x3_narrow_bwd_weight: bad arguments (1 <= nblk <= 65536)");
  TPGSR_CHECK_ARG(narrow_args_ok(N, H, W, Cin, Cout), "tpgsr_conv3x3_narrow_bwd_weight" NARROW_ARGS_MSG, N, H, W, Cin, Cout);
  const long long runs = run_count(N, H, W);
  const long long per_blk = (runs + nblk - 1) / nblk;
  const int vec = aligned16(x, partial, nullptr);
  NARROW_DISPATCH(narrow_bwd_weight_kernel, dim3(nblk), dim3(64), x, dy, N, H, W, Cin, vec, per_blk, partial);
  TPGSR_LAUNCH_CHECK("tpgsr_conv3x3_narrow_bwd_weight");
}
