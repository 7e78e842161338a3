// nn.ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1, bias=False) -- the up-sampling layer of LapSRN (reference model/lapsrn.py:48, :64).
//
// With kernel index kh = o - 2 i + 1, output row 2m reads input rows m (kh 1) and m-1 (kh 3), output row 2m+1 reads rows m (kh 2) and
// m+1 (kh 0); columns alike.  So the layer is a 3x3 pad-1 convolution to 4 Cout channels -- channel co*4 + a*2 + b for output phase
// (a, b), tap (r, s) of it holding w[kh = a - 2r + 3][kw = b - 2s + 3] where that index exists (4 of the 9 taps) -- followed by
// PixelShuffle(2): the 64 -> 256 pixel-shuffle-store convolution of the up-sampling blocks.
//
//   tpgsr_tconv4s2_expand     w [Cin][Cout][4][4] -> w3 [4 Cout][Cin][3][3] (zeros included)
//   tpgsr_tconv4s2_fold_grad  dW3 [4 Cout][Cin][3][3] -> dw [Cin][Cout][4][4] (+=)
// are the two gathers around that convolution: one-to-one on the 16 live taps, no arithmetic but the optional accumulate.
//
// For the image branch (Cin, Cout <= 4: convt_I1 / convt_I2) a matrix-core route is waste; three direct NHWC kernels:
//   tpgsr_tconv4s2_small_fwd         one thread = one input position = its 2x2 output quad, all Cout, from the 3x3 neighbourhood
//   tpgsr_tconv4s2_small_bwd_data    one thread = one input position, all Cin: the 4x4 window of dy it fed
//   tpgsr_tconv4s2_small_bwd_weight  one workgroup = a contiguous run of input positions, one thread per weight element; [nblk][Cin Cout 16]
//                                    partial sums, finished by tpgsr_reduce_partials
// Every sum runs in a fixed order: no atomics, bitwise reproducible.
#include "common.h"

namespace {

constexpr int kSmallMaxC = 4;
constexpr int kGridCap = 2048;      // memory-bound: at most ~8 workgroups per CU, grid-stride the rest

// (phase, 3x3 tap) -> 4x4 kernel index, or -1: k = a - 2 r + 3
__device__ __forceinline__ int tap_of(int a, int r) {
  const int k = a - 2 * r + 3;
  return (unsigned)k < 4u ? k : -1;
}

__device__ __forceinline__ float expand_at(const float* __restrict__ w, int Cin, int Cout, long long e) {
  const int s = (int)(e % 3), r = (int)((e / 3) % 3);
  const long long q = e / 9;
  const int ci = (int)(q % Cin), c3 = (int)(q / Cin);
  const int kh = tap_of((c3 >> 1) & 1, r), kw = tap_of(c3 & 1, s);
  if (kh < 0 || kw < 0) return 0.f;
  return w[(((size_t)ci * Cout + (c3 >> 2)) * 4 + kh) * 4 + kw];
}

__global__ __launch_bounds__(256) void tconv4s2_expand_kernel(const float* __restrict__ w, int Cin, int Cout, long long n4, long long n,
                                                              float* __restrict__ w3) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    const long long e = i * 4;
    *reinterpret_cast<float4*>(w3 + e) =
        make_float4(expand_at(w, Cin, Cout, e), expand_at(w, Cin, Cout, e + 1), expand_at(w, Cin, Cout, e + 2), expand_at(w, Cin, Cout, e + 3));
  }
  for (long long e = n4 * 4 + t0; e < n; e += stride) w3[e] = expand_at(w, Cin, Cout, e);
}

// dw element (ci, co, kh, kw) <- dW3 channel co*4 + a*2 + b, tap (r, s): a = 1 - (kh & 1), r = (3 + a - kh) / 2 (the inverse of tap_of)
__global__ __launch_bounds__(256) void tconv4s2_fold_kernel(const float* __restrict__ dw3, int Cin, int Cout, int accumulate, int vec,
                                                            long long n, float* __restrict__ dw) {
  // one thread per kernel row (ci, co, kh): the four kw of it
  const long long rows = n >> 2, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += stride) {
    const int kh = (int)(i & 3);
    const long long q = i >> 2;
    const int co = (int)(q % Cout), ci = (int)(q / Cout);
    const int a = 1 - (kh & 1), r = (3 + a - kh) >> 1;
    float v[4];
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const int b = 1 - (kw & 1), s = (3 + b - kw) >> 1;
      v[kw] = dw3[(((size_t)(co * 4 + a * 2 + b)) * Cin + ci) * 9 + r * 3 + s];
    }
    float* dst = dw + i * 4;
    if (vec) {
      float4 o = make_float4(v[0], v[1], v[2], v[3]);
      if (accumulate) {
        const float4 p = *reinterpret_cast<const float4*>(dst);
        o.x = p.x + o.x; o.y = p.y + o.y; o.z = p.z + o.z; o.w = p.w + o.w;
      }
      *reinterpret_cast<float4*>(dst) = o;
    } else {
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) dst[kw] = accumulate ? dst[kw] + v[kw] : v[kw];
    }
  }
}

// ---- the narrow direct kernels (Cin, Cout <= 4) ----
// weights in LDS as [ci][co][kh][kw] (<= 256 floats)
__device__ __forceinline__ void stage_weights(const float* __restrict__ w, int n, float* ws) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
}

__global__ __launch_bounds__(256) void tconv4s2_small_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int H, int W,
                                                                 int Cin, int Cout, float* __restrict__ y) {
  __shared__ float ws[kSmallMaxC * kSmallMaxC * 16];
  stage_weights(w, Cin * Cout * 16, ws);
  const int total = N * H * W, stride = gridDim.x * blockDim.x;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
    const int q = p % W, m = (p / W) % H, n = p / (W * H);
    float acc[4][kSmallMaxC];      // [phase a*2 + b][co]
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int co = 0; co < kSmallMaxC; ++co) acc[f][co] = 0.f;
    // fixed order: input channel, then the neighbourhood row by row
#pragma unroll
    for (int ci = 0; ci < kSmallMaxC; ++ci) {
      if (ci >= Cin) break;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int ih = m + r - 1;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int iw = q + s - 1;
          if ((unsigned)iw >= (unsigned)W) continue;
          const float xv = x[((size_t)(n * H + ih) * W + iw) * Cin + ci];
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const int kh = a - 2 * r + 3;
            if ((unsigned)kh >= 4u) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const int kw = b - 2 * s + 3;
              if ((unsigned)kw >= 4u) continue;
#pragma unroll
              for (int co = 0; co < kSmallMaxC; ++co)
                if (co < Cout) acc[a * 2 + b][co] = __builtin_fmaf(xv, ws[((ci * Cout + co) * 4 + kh) * 4 + kw], acc[a * 2 + b][co]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float* dst = y + ((size_t)(n * 2 * H + 2 * m + a) * (2 * W) + 2 * q + b) * Cout;
#pragma unroll
        for (int co = 0; co < kSmallMaxC; ++co)
          if (co < Cout) dst[co] = acc[a * 2 + b][co];
      }
  }
}

// dx[n][m][q][ci] = sum_co sum_kh sum_kw dy[n][2m - 1 + kh][2q - 1 + kw][co] * w[ci][co][kh][kw]
__global__ __launch_bounds__(256) void tconv4s2_small_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int H, int W,
                                                                      int Cin, int Cout, float* __restrict__ dx) {
  __shared__ float ws[kSmallMaxC * kSmallMaxC * 16];
  stage_weights(w, Cin * Cout * 16, ws);
  const int total = N * H * W, stride = gridDim.x * blockDim.x, OH = 2 * H, OW = 2 * W;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
    const int q = p % W, m = (p / W) % H, n = p / (W * H);
    float acc[kSmallMaxC];
#pragma unroll
    for (int ci = 0; ci < kSmallMaxC; ++ci) acc[ci] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
      const int oh = 2 * m - 1 + kh;
      if ((unsigned)oh >= (unsigned)OH) continue;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        const int ow = 2 * q - 1 + kw;
        if ((unsigned)ow >= (unsigned)OW) continue;
        const float* g = dy + ((size_t)(n * OH + oh) * OW + ow) * Cout;
#pragma unroll
        for (int co = 0; co < kSmallMaxC; ++co) {
          if (co >= Cout) break;
          const float gv = g[co];
#pragma unroll
          for (int ci = 0; ci < kSmallMaxC; ++ci)
            if (ci < Cin) acc[ci] = __builtin_fmaf(gv, ws[((ci * Cout + co) * 4 + kh) * 4 + kw], acc[ci]);
        }
      }
    }
    float* dst = dx + (size_t)p * Cin;
#pragma unroll
    for (int ci = 0; ci < kSmallMaxC; ++ci)
      if (ci < Cin) dst[ci] = acc[ci];
  }
}

// partial[blk][e], e = ((ci * Cout + co) * 4 + kh) * 4 + kw: sum over the workgroup's run of input positions [p0, p1), in order, of
// x[p][ci] * dy[n][2m - 1 + kh][2q - 1 + kw][co]
__global__ __launch_bounds__(256) void tconv4s2_small_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int H,
                                                                        int W, int Cin, int Cout, int per_blk, float* __restrict__ partial) {
  const int E = Cin * Cout * 16, e = threadIdx.x;
  if (e >= E) return;
  const int kw = e & 3, kh = (e >> 2) & 3, co = (e >> 4) % Cout, ci = (e >> 4) / Cout;
  const int total = N * H * W, OH = 2 * H, OW = 2 * W;
  const int p0 = blockIdx.x * per_blk, p1 = min(total, p0 + per_blk);
  float acc = 0.f;
  for (int p = p0; p < p1; ++p) {
    const int q = p % W, m = (p / W) % H, n = p / (W * H);
    const int oh = 2 * m - 1 + kh, ow = 2 * q - 1 + kw;
    if ((unsigned)oh < (unsigned)OH && (unsigned)ow < (unsigned)OW)
      acc = __builtin_fmaf(x[(size_t)p * Cin + ci], dy[((size_t)(n * OH + oh) * OW + ow) * Cout + co], acc);
  }
  partial[(size_t)blockIdx.x * E + e] = acc;
}

bool small_args_ok(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin < 1 || Cin > kSmallMaxC || Cout < 1 || Cout > kSmallMaxC) return false;
  // every element index of x / dx (N H W Cin) and y / dy (N 2H 2W Cout) below 2^31
  const long long pix = (long long)N * H * W;
  return pix * 4 * kSmallMaxC < (1ll << 31);
}

int capped_grid(long long work) { return (int)max((long long)1, min((long long)kGridCap, (work + 255) / 256)); }

}  // namespace

extern "C" int tpgsr_tconv4s2_expand(const float* w, int Cin, int Cout, float* w3, void* stream) {
  TPGSR_CHECK_ARG(w && w3 && Cin > 0 && Cout > 0 && (long long)Cin * Cout * 36 < (1ll << 31), "tpgsr_tconv4s2_expand: bad arguments");
  const long long n = (long long)Cin * Cout * 36;
  const long long n4 = (((uintptr_t)w3) & 15) == 0 ? n / 4 : 0;
  hipLaunchKernelGGL(tconv4s2_expand_kernel, dim3(capped_grid(n4 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, w, Cin, Cout, n4, n, w3);
  TPGSR_LAUNCH_CHECK("tpgsr_tconv4s2_expand");
}

extern "C" int tpgsr_tconv4s2_fold_grad(const float* dw3, int Cin, int Cout, float* dw, int accumulate, void* stream) {
  TPGSR_CHECK_ARG(dw3 && dw && Cin > 0 && Cout > 0 && (long long)Cin * Cout * 36 < (1ll << 31), "tpgsr_tconv4s2_fold_grad: bad arguments");
  const long long n = (long long)Cin * Cout * 16;
  const int vec = (((uintptr_t)dw) & 15) == 0;
  hipLaunchKernelGGL(tconv4s2_fold_kernel, dim3(capped_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, dw3, Cin, Cout, accumulate ? 1 : 0, vec, n,
                     dw);
  TPGSR_LAUNCH_CHECK("tpgsr_tconv4s2_fold_grad");
}

extern "C" int tpgsr_tconv4s2_small_fwd(const float* x, const float* w, int N, int H, int W, int Cin, int Cout, float* y, void* stream) {
  TPGSR_CHECK_ARG(x && w && y, "tpgsr_tconv4s2_small_fwd: null pointer");
  TPGSR_CHECK_ARG(small_args_ok(N, H, W, Cin, Cout),
                  "tpgsr_tconv4s2_small_fwd: takes 1 <= Cin, Cout <= 4 and fewer than 2^27 input positions (got N %d, H %d, W %d, Cin %d, Cout %d)", N,
                  H, W, Cin, Cout);
  hipLaunchKernelGGL(tconv4s2_small_fwd_kernel, dim3(capped_grid((long long)N * H * W)), dim3(256), 0, (hipStream_t)stream, x, w, N, H, W, Cin,
                     Cout, y);
  TPGSR_LAUNCH_CHECK("tpgsr_tconv4s2_small_fwd");
}

extern "C" int tpgsr_tconv4s2_small_bwd_data(const float* dy, const float* w, int N, int H, int W, int Cin, int Cout, float* dx, void* stream) {
  TPGSR_CHECK_ARG(dy && w && dx, "tpgsr_tconv4s2_small_bwd_data: null pointer");
  TPGSR_CHECK_ARG(small_args_ok(N, H, W, Cin, Cout),
                  "tpgsr_tconv4s2_small_bwd_data: takes 1 <= Cin, Cout <= 4 and fewer than 2^27 input positions (got N %d, H %d, W %d, Cin %d, Cout %d)",
                  N, H, W, Cin, Cout);
  hipLaunchKernelGGL(tconv4s2_small_bwd_data_kernel, dim3(capped_grid((long long)N * H * W)), dim3(256), 0, (hipStream_t)stream, dy, w, N, H, W,
                     Cin, Cout, dx);
  TPGSR_LAUNCH_CHECK("tpgsr_tconv4s2_small_bwd_data");
}

extern "C" int tpgsr_tconv4s2_small_bwd_weight(const float* x, const float* dy, int N, int H, int W, int Cin, int Cout, float* partial, int nblk,
                                               void* stream) {
  TPGSR_CHECK_ARG(x && dy && partial && nblk > 0 && nblk <= 65536, "tpgsr_tconv4s2_small_bwd_weight: bad arguments (1 <= nblk <= 65536)");
  TPGSR_CHECK_ARG(small_args_ok(N, H, W, Cin, Cout),
                  "tpgsr_tconv4s2_small_bwd_weight: takes 1 <= Cin, Cout <= 4 and fewer than 2^27 input positions (got N %d, H %d, W %d, Cin %d, Cout %d)",
                  N, H, W, Cin, Cout);
  const long long total = (long long)N * H * W;
  const int per_blk = (int)((total + nblk - 1) / nblk);      // (workgroups past the end write zeros: every row of partial is defined)
  hipLaunchKernelGGL(tconv4s2_small_bwd_weight_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, dy, N, H, W, Cin, Cout, per_blk, partial);
  TPGSR_LAUNCH_CHECK("tpgsr_tconv4s2_small_bwd_weight");
}
