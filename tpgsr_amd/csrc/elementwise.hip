// HBM-bound elementwise / per-channel reduction kernels: train-mode BatchNorm (statistics, backward),
// activation + max-pool materialisation (STN head), PReLU, layout transposes, small reductions.
// All tensors are [M][C] row-major (NHWC flattened); channel loops are float4-vectorised when C % 4 == 0.
#include "common.h"
#include <type_traits>

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ------------------------------------------------------------------------------------------------------
// BatchNorm statistics
// ------------------------------------------------------------------------------------------------------
// partial[b][0][c] = sum_m x, partial[b][1][c] = sum_m x^2 over the rows of block b
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, long long M, int C, int ld,
                                                       float* __restrict__ partial, int nblk) {
  long long rows_per = (M + nblk - 1) / nblk;
  long long r0 = blockIdx.x * rows_per, r1 = min(M, r0 + rows_per);
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f, ss = 0.f;
    for (long long r = r0; r < r1; ++r) {
      float v = x[r * ld + c];
      s += v;
      ss += v * v;
    }
    partial[((size_t)blockIdx.x * 2 + 0) * C + c] = s;
    partial[((size_t)blockIdx.x * 2 + 1) * C + c] = ss;
  }
}

extern "C" int tpgsr_bn_stats(const float* x, long long M, int C, int ld, float* partial, int nblk, void* stream) {
  TPGSR_CHECK_ARG(x && partial && M > 0 && C > 0 && nblk > 0, "tpgsr_bn_stats: bad arguments");
  hipLaunchKernelGGL(bn_stats_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, M, C, ld, partial, nblk);
  TPGSR_LAUNCH_CHECK("tpgsr_bn_stats");
}

// per-channel sum of the two partial rows [nblk][2][C] in fp64: one workgroup per channel, 256 row lanes (every lane issues
// its <= nblk/256 loads back to back), wave shuffle + 4-entry LDS combine in a fixed order.  (16 channels x 16 row
// slices per workgroup = 4 workgroups for C = 64 took 12-16 us: each thread walked 48 partial rows serially.)
__device__ __forceinline__ void channel_sums(const float* __restrict__ partial, int nblk, int C, int c, double& s, double& ss) {
  __shared__ double red[2][4];
  double a = 0.0, b2 = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) {
    a += (double)partial[((size_t)b * 2 + 0) * C + c];
    b2 += (double)partial[((size_t)b * 2 + 1) * C + c];
  }
  a = wave_sum_d(a);
  b2 = wave_sum_d(b2);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b2;
  }
  __syncthreads();
  s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  ss = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, int nblk, int C,
                                                          long long count, const float* conv_bias,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* running_mean, float* running_var, float momentum,
                                                          float eps, int eval, float* scale, float* shift,
                                                          float* save_mean, float* save_rstd) {
  const int c = blockIdx.x;
  if (eval) {
    if (threadIdx.x == 0) {
      float rstd = 1.f / sqrtf(running_var[c] + eps);
      float sc = gamma[c] * rstd;
      scale[c] = sc;
      shift[c] = beta[c] - running_mean[c] * sc;
    }
    return;
  }
  double s, ss;
  channel_sums(partial, nblk, C, c, s, ss);
  if (threadIdx.x == 0) {
    double mean_raw = s / (double)count;
    double var = ss / (double)count - mean_raw * mean_raw;
    if (var < 0.0) var = 0.0;
    double mean = mean_raw + (conv_bias ? (double)conv_bias[c] : 0.0);
    double rstd = 1.0 / sqrt(var + (double)eps);
    float sc = (float)((double)gamma[c] * rstd);
    scale[c] = sc;
    shift[c] = (float)((double)beta[c] - mean * (double)gamma[c] * rstd);
    if (save_mean) save_mean[c] = (float)mean;
    if (save_rstd) save_rstd[c] = (float)rstd;
    if (running_mean) {
      double unbiased = count > 1 ? var * (double)count / (double)(count - 1) : var;
      running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
      running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    }
  }
}

extern "C" int tpgsr_bn_finalize(const float* partial, int nblk, int C, long long count, const float* conv_bias,
                                 const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 float momentum, float eps, int eval, float* scale, float* shift, float* save_mean,
                                 float* save_rstd, void* stream) {
  TPGSR_CHECK_ARG(gamma && beta && scale && shift && C > 0, "tpgsr_bn_finalize: null pointer");
  TPGSR_CHECK_ARG(eval || (partial && nblk > 0 && count > 0), "tpgsr_bn_finalize: training mode needs partial statistics");
  TPGSR_CHECK_ARG(!eval || (running_mean && running_var), "tpgsr_bn_finalize: eval mode needs running statistics");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, partial, nblk, C, count,
                     conv_bias, gamma, beta, running_mean, running_var, momentum, eps, eval, scale, shift, save_mean,
                     save_rstd);
  TPGSR_LAUNCH_CHECK("tpgsr_bn_finalize");
}

// ------------------------------------------------------------------------------------------------------
// BatchNorm (+activation) backward
//   z = scale*y + shift ; a = act(z) ; given da (+da2): dz = da*act'(z)
//   pass 1: partial[b][0][c] = sum dz ; partial[b][1][c] = sum dz*xhat, xhat = (y-mean)*rstd
//   pass 2: dy = coef0*dz + coef1*y + coef2
// thread layout: C4 = C/4 channel quads across threads, 256/C4 row lanes; requires C%4==0, 256%(C/4)==0
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ da, const float* __restrict__ da2,
                                                            const float* __restrict__ y, long long M, int C,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ save_mean,
                                                            const float* __restrict__ save_rstd, int act,
                                                            float* __restrict__ partial, int nblk) {
  extern __shared__ float sm[];  // [rowlanes][2][C]
  const int C4 = C >> 2;
  const int rl = 256 / C4;
  const int q = threadIdx.x % C4, lane_r = threadIdx.x / C4;
  const int c = q * 4;
  long long rows_per = (M + nblk - 1) / nblk;
  long long r0 = blockIdx.x * rows_per, r1 = min(M, r0 + rows_per);
  float4 sc = ld4(scale + c), sh = ld4(shift + c), mu = ld4(save_mean + c), rs = ld4(save_rstd + c);
  float4 s = make_float4(0, 0, 0, 0), sx = make_float4(0, 0, 0, 0);
  // four rows' loads in flight per thread (the loop is latency-bound: a block owns ~64 rows, 4 per thread); the sums run in the
  // same order as a row-at-a-time loop, rows past the end contribute +0.  Two instances (with / without the second gradient
  // operand) so that no branch -- and with it a full s_waitcnt -- sits between the loads.
  constexpr int U = 4;
  auto sweep = [&](auto has2_tag) __attribute__((always_inline)) {
    constexpr bool HAS2 = decltype(has2_tag)::value;
    for (long long r = r0 + lane_r; r < r1; r += (long long)U * rl) {
      float4 g[U], g2[HAS2 ? U : 1], yv[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long rr = r + (long long)u * rl;
        ok[u] = rr < r1;
        const long long o = (ok[u] ? rr : r) * C + c;
        g[u] = ld4(da + o);
        if (HAS2) g2[u] = ld4(da2 + o);
        yv[u] = ld4(y + o);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (HAS2) {
          g[u].x += g2[u].x; g[u].y += g2[u].y; g[u].z += g2[u].z; g[u].w += g2[u].w;
        }
        if (!ok[u]) g[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (act) {
          g[u].x *= act_grad(yv[u].x * sc.x + sh.x, act);
          g[u].y *= act_grad(yv[u].y * sc.y + sh.y, act);
          g[u].z *= act_grad(yv[u].z * sc.z + sh.z, act);
          g[u].w *= act_grad(yv[u].w * sc.w + sh.w, act);
        }
        s.x += g[u].x; s.y += g[u].y; s.z += g[u].z; s.w += g[u].w;
        sx.x += g[u].x * (yv[u].x - mu.x) * rs.x;
        sx.y += g[u].y * (yv[u].y - mu.y) * rs.y;
        sx.z += g[u].z * (yv[u].z - mu.z) * rs.z;
        sx.w += g[u].w * (yv[u].w - mu.w) * rs.w;
      }
    }
  };
  if (da2) sweep(std::true_type{}); else sweep(std::false_type{});
  float* a0 = sm + ((size_t)lane_r * 2 + 0) * C + c;
  float* a1 = sm + ((size_t)lane_r * 2 + 1) * C + c;
  *reinterpret_cast<float4*>(a0) = s;
  *reinterpret_cast<float4*>(a1) = sx;
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    float t = 0.f;
    for (int l = 0; l < rl; ++l) t += sm[(size_t)l * 2 * C + i];
    partial[(size_t)blockIdx.x * 2 * C + i] = t;
  }
}

static int bn_vec_ok(int C) { return (C & 3) == 0 && C >= 4 && C <= 1024 && (256 % (C >> 2)) == 0; }

extern "C" int tpgsr_bn_bwd_reduce(const float* da, const float* da2, const float* y, long long M, int C,
                                   const float* scale, const float* shift, const float* save_mean,
                                   const float* save_rstd, int act, float* partial, int nblk, void* stream) {
  TPGSR_CHECK_ARG(da && y && scale && shift && save_mean && save_rstd && partial && nblk > 0, "tpgsr_bn_bwd_reduce: null pointer");
  TPGSR_CHECK_ARG(bn_vec_ok(C), "tpgsr_bn_bwd_reduce: unsupported channel count %d", C);
  size_t smem = (size_t)(256 / (C >> 2)) * 2 * C * sizeof(float);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk), dim3(256), smem, (hipStream_t)stream, da, da2, y, M, C, scale, shift,
                     save_mean, save_rstd, act, partial, nblk);
  TPGSR_LAUNCH_CHECK("tpgsr_bn_bwd_reduce");
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nblk, int C,
                                                              long long count, const float* __restrict__ gamma,
                                                              const float* __restrict__ save_mean,
                                                              const float* __restrict__ save_rstd, float* dgamma,
                                                              float* dbeta, int accumulate, float* coef) {
  const int c = blockIdx.x;
  double s, sx;
  channel_sums(partial, nblk, C, c, s, sx);
  if (threadIdx.x == 0) {
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)sx : (float)sx;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s : (float)s;
    double rstd = save_rstd[c], mu = save_mean[c], g = gamma[c];
    double mdz = s / (double)count, mdzx = sx / (double)count;
    double c0 = g * rstd;
    coef[c] = (float)c0;
    coef[C + c] = (float)(-c0 * mdzx * rstd);
    coef[2 * C + c] = (float)(-c0 * (mdz - mu * rstd * mdzx));
  }
}

extern "C" int tpgsr_bn_bwd_finalize(const float* partial, int nblk, int C, long long count, const float* gamma,
                                     const float* save_mean, const float* save_rstd, float* dgamma, float* dbeta,
                                     int accumulate, float* coef, void* stream) {
  TPGSR_CHECK_ARG(partial && gamma && save_mean && save_rstd && coef && nblk > 0 && count > 0, "tpgsr_bn_bwd_finalize: bad arguments");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, partial, nblk, C, count,
                     gamma, save_mean, save_rstd, dgamma, dbeta, accumulate, coef);
  TPGSR_LAUNCH_CHECK("tpgsr_bn_bwd_finalize");
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ da, const float* __restrict__ da2,
                                                           const float* __restrict__ y, long long total4, int C,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           int act, const float* __restrict__ coef, float* __restrict__ dy) {
  const int C4 = C >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C4) * 4;
    float4 g = ld4(da + i * 4);
    if (da2) {
      float4 g2 = ld4(da2 + i * 4);
      g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
    }
    float4 yv = ld4(y + i * 4);
    if (act) {
      float4 sc = ld4(scale + c), sh = ld4(shift + c);
      g.x *= act_grad(yv.x * sc.x + sh.x, act);
      g.y *= act_grad(yv.y * sc.y + sh.y, act);
      g.z *= act_grad(yv.z * sc.z + sh.z, act);
      g.w *= act_grad(yv.w * sc.w + sh.w, act);
    }
    float4 c0 = ld4(coef + c), c1 = ld4(coef + C + c), c2 = ld4(coef + 2 * C + c);
    float4 o;
    o.x = c0.x * g.x + c1.x * yv.x + c2.x;
    o.y = c0.y * g.y + c1.y * yv.y + c2.y;
    o.z = c0.z * g.z + c1.z * yv.z + c2.z;
    o.w = c0.w * g.w + c1.w * yv.w + c2.w;
    *reinterpret_cast<float4*>(dy + i * 4) = o;
  }
}

extern "C" int tpgsr_bn_bwd_apply(const float* da, const float* da2, const float* y, long long M, int C, const float* scale,
                                  const float* shift, int act, const float* coef, float* dy, void* stream) {
  TPGSR_CHECK_ARG(da && y && coef && dy && (C & 3) == 0, "tpgsr_bn_bwd_apply: bad arguments");
  TPGSR_CHECK_ARG(!act || (scale && shift), "tpgsr_bn_bwd_apply: activation needs scale/shift");
  long long total4 = M * C / 4;
  int grid = (int)min((long long)4096, (total4 + 255) / 256);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, da, da2, y, total4, C, scale, shift,
                     act, coef, dy);
  TPGSR_LAUNCH_CHECK("tpgsr_bn_bwd_apply");
}

// out = act(scale[c]*x + shift[c]) materialised once (float4-vectorised): used where the consumer would otherwise
// re-apply an expensive activation per filter tap (mish in front of a 3x3 / 9x1 conv)
__global__ __launch_bounds__(256) void affine_act_kernel(const float* __restrict__ x, long long total4, int C,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         int act, float* __restrict__ out) {
  const int C4 = C >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = ld4(x + i * 4);
    if (scale) {
      int c = (int)(i % C4) * 4;
      float4 s = ld4(scale + c), t = ld4(shift + c);
      v.x = v.x * s.x + t.x; v.y = v.y * s.y + t.y; v.z = v.z * s.z + t.z; v.w = v.w * s.w + t.w;
    }
    v.x = apply_act(v.x, act); v.y = apply_act(v.y, act); v.z = apply_act(v.z, act); v.w = apply_act(v.w, act);
    *reinterpret_cast<float4*>(out + i * 4) = v;
  }
}

__global__ void affine_act_pool_kernel(const float* __restrict__ x, int N, int H, int W, int C, const float* __restrict__ scale,
                                       const float* __restrict__ shift, int act, int ph, int pw, float* __restrict__ out);

extern "C" int tpgsr_affine_act(const float* x, long long M, int C, const float* scale, const float* shift, int act, float* out,
                                void* stream) {
  TPGSR_CHECK_ARG(x && out && M > 0 && C > 0, "tpgsr_affine_act: bad arguments");
  TPGSR_CHECK_ARG((scale == nullptr) == (shift == nullptr), "tpgsr_affine_act: scale/shift must come together");
  if (C & 3) {   // channel counts that are no multiple of 4 (the one-channel offset map of MORAN's rectifier): the scalar 1x1 "pool"
    TPGSR_CHECK_ARG(M < (1ll << 31), "tpgsr_affine_act: M too large for the scalar path");
    const long long total = M * C;
    const int grid = (int)min((long long)4096, (total + 255) / 256);
    hipLaunchKernelGGL(affine_act_pool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, 1, 1, (int)M, C, scale, shift, act, 1, 1, out);
    TPGSR_LAUNCH_CHECK("tpgsr_affine_act");
  }
  long long total4 = M * C / 4;
  int grid = (int)min((long long)8192, (total4 + 255) / 256);
  hipLaunchKernelGGL(affine_act_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, total4, C, scale, shift, act, out);
  TPGSR_LAUNCH_CHECK("tpgsr_affine_act");
}

// ------------------------------------------------------------------------------------------------------
// act(scale*x+shift) + max-pool (ph x pw, stride = window, floor) -- STN head / CRNN pooling stages
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void affine_act_pool_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int act, int ph, int pw,
                                                              float* __restrict__ out) {
  int OH = H / ph, OW = W / pw;
  long long total = (long long)N * OH * OW * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long p = i / C;
    int ow = (int)(p % OW);
    p /= OW;
    int oh = (int)(p % OH);
    int n = (int)(p / OH);
    float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    float best = -INFINITY;
    for (int a = 0; a < ph; ++a)
      for (int b = 0; b < pw; ++b) {
        float v = x[((size_t)(n * H + oh * ph + a) * W + ow * pw + b) * C + c];
        v = apply_act(v * sc + sh, act);
        if (v > best || v != v) best = v;
      }
    out[i] = best;
  }
}

extern "C" int tpgsr_affine_act_pool(const float* x, int N, int H, int W, int C, const float* scale, const float* shift,
                                     int act, int pool_h, int pool_w, float* out, void* stream) {
  TPGSR_CHECK_ARG(x && out && pool_h >= 1 && pool_w >= 1 && H >= pool_h && W >= pool_w, "tpgsr_affine_act_pool: bad arguments");
  long long total = (long long)N * (H / pool_h) * (W / pool_w) * C;
  int grid = (int)min((long long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(affine_act_pool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, N, H, W, C, scale, shift, act,
                     pool_h, pool_w, out);
  TPGSR_LAUNCH_CHECK("tpgsr_affine_act_pool");
}

// dz[n][h][w][c] = (h,w is the first arg-max of its window) ? dout * act'(scale*x+shift) : 0
__global__ __launch_bounds__(256) void affine_act_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout,
                                                                  int N, int H, int W, int C,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift, int act, int ph, int pw,
                                                                  float* __restrict__ dz) {
  int OH = H / ph, OW = W / pw;
  long long total = (long long)N * OH * OW * C;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long p = i / C;
    int ow = (int)(p % OW);
    p /= OW;
    int oh = (int)(p % OH);
    int n = (int)(p / OH);
    float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
    float best = -INFINITY, bestpre = 0.f;
    int ba = 0, bb = 0;
    for (int a = 0; a < ph; ++a)
      for (int b = 0; b < pw; ++b) {
        float pre = x[((size_t)(n * H + oh * ph + a) * W + ow * pw + b) * C + c] * sc + sh;
        float v = apply_act(pre, act);
        if (v > best || v != v) {
          best = v;
          bestpre = pre;
          ba = a;
          bb = b;
        }
      }
    float g = dout[i] * act_grad(bestpre, act);
    for (int a = 0; a < ph; ++a)
      for (int b = 0; b < pw; ++b)
        dz[((size_t)(n * H + oh * ph + a) * W + ow * pw + b) * C + c] = (a == ba && b == bb) ? g : 0.f;
  }
  // rows/cols dropped by the floor (H % ph, W % pw) receive no gradient
  if (H % ph || W % pw) {
    long long tot2 = (long long)N * H * W * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < tot2; i += (long long)gridDim.x * blockDim.x) {
      long long p = i / C;
      int w = (int)(p % W);
      int h = (int)((p / W) % H);
      if (h >= OH * ph || w >= OW * pw) dz[i] = 0.f;
    }
  }
}

extern "C" int tpgsr_affine_act_pool_bwd(const float* x, const float* dout, int N, int H, int W, int C, const float* scale,
                                         const float* shift, int act, int pool_h, int pool_w, float* dz, void* stream) {
  TPGSR_CHECK_ARG(x && dout && dz && pool_h >= 1 && pool_w >= 1, "tpgsr_affine_act_pool_bwd: bad arguments");
  long long total = (long long)N * (H / pool_h) * (W / pool_w) * C;
  int grid = (int)min((long long)4096, (total + 255) / 256);
  hipLaunchKernelGGL(affine_act_pool_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, dout, N, H, W, C, scale,
                     shift, act, pool_h, pool_w, dz);
  TPGSR_LAUNCH_CHECK("tpgsr_affine_act_pool_bwd");
}

// ------------------------------------------------------------------------------------------------------
// text-prior strip: bilinear (align_corners=True) resample along W of act(scale*in+shift), and its backward
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void strip_src(int ow, int Win, int Wout, int& x0, int& x1, float& l) {
  float sx = Wout > 1 ? (float)ow * ((float)(Win - 1) / (float)(Wout - 1)) : 0.f;
  x0 = (int)sx;
  if (x0 > Win - 1) x0 = Win - 1;
  x1 = x0 + 1 < Win ? x0 + 1 : x0;
  l = sx - (float)x0;
}

__global__ __launch_bounds__(256) void strip_resample_fwd_kernel(const float* __restrict__ in, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int act, int N, int Win,
                                                                 int Wout, int C, float* __restrict__ out) {
  long long total = (long long)N * Wout * C;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int c = (int)(i % C);
  long long r = i / C;
  int ow = (int)(r % Wout);
  int n = (int)(r / Wout);
  int x0, x1;
  float l;
  strip_src(ow, Win, Wout, x0, x1, l);
  float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  float a = apply_act(in[((size_t)n * Win + x0) * C + c] * sc + sh, act);
  float b = apply_act(in[((size_t)n * Win + x1) * C + c] * sc + sh, act);
  out[i] = a * (1.f - l) + b * l;
}

extern "C" int tpgsr_strip_resample_fwd(const float* in, const float* scale, const float* shift, int act, int N, int Win, int Wout,
                                        int C, float* out, void* stream) {
  TPGSR_CHECK_ARG(in && out && N > 0 && Win > 0 && Wout > 0 && C > 0, "tpgsr_strip_resample_fwd: bad arguments");
  long long total = (long long)N * Wout * C;
  hipLaunchKernelGGL(strip_resample_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, in, scale, shift, act, N,
                     Win, Wout, C, out);
  TPGSR_LAUNCH_CHECK("tpgsr_strip_resample_fwd");
}

// gather form (deterministic): every input column sums the output columns that sampled it
__global__ __launch_bounds__(256) void strip_resample_bwd_kernel(const float* __restrict__ in, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int act,
                                                                 const float* __restrict__ dout, int N, int Win, int Wout, int C,
                                                                 float* __restrict__ dz) {
  long long total = (long long)N * Win * C;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int c = (int)(i % C);
  long long r = i / C;
  int iw = (int)(r % Win);
  int n = (int)(r / Win);
  float g = 0.f;
  // only outputs whose two source columns include iw contribute: sx(ow) = ow (Win-1)/(Wout-1) in [iw - 1, iw + 1).  The loop visits that
  // window (+ one output either side against rounding) in ascending ow with the forward pass's own strip_src -- the same addends in the
  // same order as the full 0 .. Wout-1 sweep it replaces (27 us for a 1 MB tensor: Wout dependent loads and divisions per element)
  int lo = 0, hi = Wout - 1;
  if (Win > 1 && Wout > 1) {
    const float inv = (float)(Wout - 1) / (float)(Win - 1);
    lo = max(0, (int)floorf((float)(iw - 1) * inv) - 1);
    hi = min(Wout - 1, (int)ceilf((float)(iw + 1) * inv) + 1);
  }
  for (int ow = lo; ow <= hi; ++ow) {
    int x0, x1;
    float l;
    strip_src(ow, Win, Wout, x0, x1, l);
    float d = dout[((size_t)n * Wout + ow) * C + c];
    if (x0 == iw) g += d * (1.f - l);
    if (x1 == iw) g += d * l;
  }
  float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  dz[i] = g * act_grad(in[i] * sc + sh, act);
}

extern "C" int tpgsr_strip_resample_bwd(const float* in, const float* scale, const float* shift, int act, const float* dout, int N,
                                        int Win, int Wout, int C, float* dz, void* stream) {
  TPGSR_CHECK_ARG(in && dout && dz && N > 0 && Win > 0 && Wout > 0 && C > 0, "tpgsr_strip_resample_bwd: bad arguments");
  long long total = (long long)N * Win * C;
  hipLaunchKernelGGL(strip_resample_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, in, scale, shift, act,
                     dout, N, Win, Wout, C, dz);
  TPGSR_LAUNCH_CHECK("tpgsr_strip_resample_bwd");
}

// dstrip[n][w][c] (+)= sum_h d[n][h][w][c]: one thread per float4 of a strip row, the H loads issued together (the sum runs h = 0 .. H-1)
__global__ __launch_bounds__(256) void hsum_kernel(const float* __restrict__ d, int N, int H, int WC4, float* dstrip, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * WC4) return;
  const int n = i / WC4, wc = i - n * WC4;
  const float4* src = reinterpret_cast<const float4*>(d) + (size_t)n * H * WC4 + wc;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int h = 0;
  for (; h + 8 <= H; h += 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(h + u) * WC4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
    }
  }
  for (; h < H; ++h) {
    const float4 v = src[(size_t)h * WC4];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  float4* dst = reinterpret_cast<float4*>(dstrip) + i;
  if (accumulate) {
    const float4 o = *dst;
    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
  }
  *dst = s;
}

extern "C" int tpgsr_hsum(const float* d, int N, int H, int W, int C, float* dstrip, int accumulate, void* stream) {
  TPGSR_CHECK_ARG(d && dstrip && N > 0 && H > 0 && W > 0 && C > 0, "tpgsr_hsum: bad arguments");
  TPGSR_CHECK_ARG(((W * C) & 3) == 0 && ((((uintptr_t)d) | ((uintptr_t)dstrip)) & 15) == 0 && (long long)N * W * C < (1ll << 31),
                  "tpgsr_hsum: needs W C %% 4 == 0, 16-byte aligned operands and fewer than 2^31 strip elements");
  const int WC4 = (W * C) >> 2;
  hipLaunchKernelGGL(hsum_kernel, dim3(cdiv((long long)N * WC4, 256)), dim3(256), 0, (hipStream_t)stream, d, N, H, WC4, dstrip, accumulate);
  TPGSR_LAUNCH_CHECK("tpgsr_hsum");
}

// ------------------------------------------------------------------------------------------------------
// PReLU (single shared slope), add, activation backward, transposes, small reductions
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prelu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                        long long n4, float* __restrict__ y) {
  float a = alpha[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = ld4(x + i * 4);
    v.x = v.x > 0.f ? v.x : a * v.x;
    v.y = v.y > 0.f ? v.y : a * v.y;
    v.z = v.z > 0.f ? v.z : a * v.z;
    v.w = v.w > 0.f ? v.w : a * v.w;
    *reinterpret_cast<float4*>(y + i * 4) = v;
  }
}

extern "C" int tpgsr_prelu_fwd(const float* x, const float* alpha, long long n, float* y, void* stream) {
  TPGSR_CHECK_ARG(x && alpha && y && (n & 3) == 0, "tpgsr_prelu_fwd: bad arguments (n must be a multiple of 4)");
  int grid = (int)min((long long)4096, (n / 4 + 255) / 256);
  hipLaunchKernelGGL(prelu_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, alpha, n / 4, y);
  TPGSR_LAUNCH_CHECK("tpgsr_prelu_fwd");
}

__global__ __launch_bounds__(256) void prelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                        const float* __restrict__ dy, const float* __restrict__ dy2,
                                                        long long n4, float* __restrict__ dx, float* __restrict__ dap) {
  __shared__ double red[4];
  float a = alpha[0];
  double acc = 0.0;      // d alpha = sum over the negative side of dy * x: a heavily cancelling sum, accumulated in fp64
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = ld4(x + i * 4);
    float4 g = ld4(dy + i * 4);
    if (dy2) {
      float4 g2 = ld4(dy2 + i * 4);
      g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
    }
    float4 o;
    o.x = v.x > 0.f ? g.x : a * g.x;
    o.y = v.y > 0.f ? g.y : a * g.y;
    o.z = v.z > 0.f ? g.z : a * g.z;
    o.w = v.w > 0.f ? g.w : a * g.w;
    acc += (double)((v.x > 0.f ? 0.f : g.x * v.x) + (v.y > 0.f ? 0.f : g.y * v.y)) +
           (double)((v.z > 0.f ? 0.f : g.z * v.z) + (v.w > 0.f ? 0.f : g.w * v.w));
    *reinterpret_cast<float4*>(dx + i * 4) = o;
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) dap[blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

extern "C" int tpgsr_prelu_bwd(const float* x, const float* alpha, const float* dy, const float* dy2, long long n, float* dx,
                               float* dalpha_partial, int nblk, void* stream) {
  TPGSR_CHECK_ARG(x && alpha && dy && dx && dalpha_partial && nblk > 0 && (n & 3) == 0, "tpgsr_prelu_bwd: bad arguments");
  hipLaunchKernelGGL(prelu_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, alpha, dy, dy2, n / 4, dx,
                     dalpha_partial);
  TPGSR_LAUNCH_CHECK("tpgsr_prelu_bwd");
}

// nn.LeakyReLU(slope) (the activation of LapSRN, model/lapsrn.py:29): y = x > 0 ? x : x * slope; dx = x > 0 ? dy : dy * slope (the derivative
// at x <= 0 is `slope`, as ATen's).  Any n: 16-byte accesses while every pointer is 16-byte aligned (n4 groups), the rest element by element.
__device__ __forceinline__ float leaky(float x, float v, float slope) { return x > 0.f ? v : v * slope; }

__global__ __launch_bounds__(256) void leaky_relu_kernel(const float* __restrict__ x, const float* __restrict__ dy, long long n4, long long n,
                                                         float slope, float* __restrict__ out) {
  // dy == nullptr: the forward pass (out = leaky(x)); else the backward pass (out = dy scaled on the non-positive side of x)
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    const float4 v = ld4(x + i * 4), g = dy ? ld4(dy + i * 4) : v;
    *reinterpret_cast<float4*>(out + i * 4) = make_float4(leaky(v.x, g.x, slope), leaky(v.y, g.y, slope), leaky(v.z, g.z, slope), leaky(v.w, g.w, slope));
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) out[i] = leaky(x[i], dy ? dy[i] : x[i], slope);
}

static int leaky_launch(const float* x, const float* dy, long long n, float slope, float* out, void* stream) {
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)dy) | ((uintptr_t)out)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0, work = n4 > n - 4 * n4 ? n4 : n - 4 * n4;
  const int grid = (int)max((long long)1, min((long long)4096, (work + 255) / 256));
  hipLaunchKernelGGL(leaky_relu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, dy, n4, n, slope, out);
  return 0;
}

extern "C" int tpgsr_leaky_relu_fwd(const float* x, long long n, float slope, float* y, void* stream) {
  TPGSR_CHECK_ARG(x && y && n > 0, "tpgsr_leaky_relu_fwd: bad arguments");
  leaky_launch(x, nullptr, n, slope, y, stream);
  TPGSR_LAUNCH_CHECK("tpgsr_leaky_relu_fwd");
}

extern "C" int tpgsr_leaky_relu_bwd(const float* x, const float* dy, long long n, float slope, float* dx, void* stream) {
  TPGSR_CHECK_ARG(x && dy && dx && n > 0, "tpgsr_leaky_relu_bwd: bad arguments");
  leaky_launch(x, dy, n, slope, dx, stream);
  TPGSR_LAUNCH_CHECK("tpgsr_leaky_relu_bwd");
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n4,
                                                  long long n, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 u = ld4(a + i * 4), v = ld4(b + i * 4);
    u.x += v.x; u.y += v.y; u.z += v.z; u.w += v.w;
    *reinterpret_cast<float4*>(out + i * 4) = u;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    long long i = n4 * 4 + threadIdx.x;
    out[i] = a[i] + b[i];
  }
}

extern "C" int tpgsr_add(const float* a, const float* b, long long n, float* out, void* stream) {
  TPGSR_CHECK_ARG(a && b && out && n > 0, "tpgsr_add: bad arguments");
  int grid = (int)max((long long)1, min((long long)4096, (n / 4 + 255) / 256));
  hipLaunchKernelGGL(add_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, n / 4, n, out);
  TPGSR_LAUNCH_CHECK("tpgsr_add");
}

// out = ((a0 + a1) + a2) + ... + a[k-1], 2 <= k <= 8: the gradient of a tensor with k consumers (functional.fork) in ONE launch.  Every
// element is summed left to right in fp32 -- plain adds, nothing for the compiler to contract or reassociate -- so the result does not
// depend on the grid or on the vector / scalar split: bitwise the host loop `s = a0; s += a1; ...`.  16-byte loads while every pointer is
// 16-byte aligned (n4 = n / 4 groups, else n4 = 0), the rest element by element.
struct add_n_ptrs {
  const float* p[8];
};

__global__ __launch_bounds__(256) void add_n_kernel(add_n_ptrs a, int k, long long n4, long long n, float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = t0; i < n4; i += stride) {
    float4 s = *reinterpret_cast<const float4*>(a.p[0] + i * 4);
#pragma unroll
    for (int j = 1; j < 8; ++j) {      // (unrolled over the constant bound: the pointers stay in scalar registers; k is uniform)
      if (j < k) {
        const float4 v = *reinterpret_cast<const float4*>(a.p[j] + i * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
    }
    *reinterpret_cast<float4*>(out + i * 4) = s;
  }
  for (long long i = n4 * 4 + t0; i < n; i += stride) {
    float s = a.p[0][i];
#pragma unroll
    for (int j = 1; j < 8; ++j)
      if (j < k) s += a.p[j][i];
    out[i] = s;
  }
}

extern "C" int tpgsr_add_n(const float* a0, const float* a1, const float* a2, const float* a3, const float* a4, const float* a5,
                           const float* a6, const float* a7, int k, long long n, float* out, void* stream) {
  const float* in[8] = {a0, a1, a2, a3, a4, a5, a6, a7};
  TPGSR_CHECK_ARG(out && n > 0 && k >= 2 && k <= 8, "tpgsr_add_n: bad arguments (2 <= k <= 8 addends, n > 0)");
  add_n_ptrs a;
  bool vec = (((uintptr_t)out) & 15) == 0;
  for (int j = 0; j < 8; ++j) {
    TPGSR_CHECK_ARG(j >= k || in[j], "tpgsr_add_n: addend %d of %d is a null pointer", j, k);
    a.p[j] = j < k ? in[j] : nullptr;
    if (j < k) vec = vec && (((uintptr_t)in[j]) & 15) == 0;
  }
  const long long n4 = vec ? n / 4 : 0;
  const long long work = n4 > (n - 4 * n4) ? n4 : n - 4 * n4;
  int grid = (int)max((long long)1, min((long long)4096, (work + 255) / 256));
  hipLaunchKernelGGL(add_n_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, k, n4, n, out);
  TPGSR_LAUNCH_CHECK("tpgsr_add_n");
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float* x, const float* dy, long long n, int act, float* dx) {
  long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 xv = ld4(x + i * 4), g = ld4(dy + i * 4);
    g.x *= act_grad(xv.x, act); g.y *= act_grad(xv.y, act); g.z *= act_grad(xv.z, act); g.w *= act_grad(xv.w, act);
    *reinterpret_cast<float4*>(dx + i * 4) = g;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    long long i = n4 * 4 + threadIdx.x;
    dx[i] = dy[i] * act_grad(x[i], act);
  }
}

extern "C" int tpgsr_act_bwd(const float* x, const float* dy, long long n, int act, float* dx, void* stream) {
  TPGSR_CHECK_ARG(x && dy && dx && n > 0, "tpgsr_act_bwd: bad arguments");
  int grid = (int)max((long long)1, min((long long)8192, (n / 4 + 255) / 256));
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, dy, n, act, dx);
  TPGSR_LAUNCH_CHECK("tpgsr_act_bwd");
}

__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, int N, int C, int HW,
                                                           float* __restrict__ out) {
  long long total = (long long)N * C * HW;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long long p = i / C;
    int hw = (int)(p % HW);
    int n = (int)(p / HW);
    out[i] = in[((size_t)n * C + c) * HW + hw];
  }
}
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ in, int N, int C, int HW,
                                                           float* __restrict__ out) {
  long long total = (long long)N * C * HW;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int hw = (int)(i % HW);
    long long p = i / HW;
    int c = (int)(p % C);
    int n = (int)(p / C);
    out[i] = in[((size_t)n * HW + hw) * C + c];
  }
}

extern "C" int tpgsr_nchw_to_nhwc(const float* in, int N, int C, int H, int W, float* out, void* stream) {
  TPGSR_CHECK_ARG(in && out && N > 0 && C > 0 && H > 0 && W > 0, "tpgsr_nchw_to_nhwc: bad arguments");
  long long total = (long long)N * C * H * W;
  int grid = (int)min((long long)8192, (total + 255) / 256);
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, N, C, H * W, out);
  TPGSR_LAUNCH_CHECK("tpgsr_nchw_to_nhwc");
}
extern "C" int tpgsr_nhwc_to_nchw(const float* in, int N, int C, int H, int W, float* out, void* stream) {
  TPGSR_CHECK_ARG(in && out && N > 0 && C > 0 && H > 0 && W > 0, "tpgsr_nhwc_to_nchw: bad arguments");
  long long total = (long long)N * C * H * W;
  int grid = (int)min((long long)8192, (total + 255) / 256);
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, N, C, H * W, out);
  TPGSR_LAUNCH_CHECK("tpgsr_nhwc_to_nchw");
}

// one block per output: 256 lanes stride over the Z partials, fixed-order tree combine (deterministic)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ part, int Z, int n, float* out,
                                                              int accumulate) {
  __shared__ double red[4];
  const int i = blockIdx.x;
  double s = 0.0;
  for (int z = threadIdx.x; z < Z; z += 256) s += (double)part[(size_t)z * n + i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = (float)((red[0] + red[1]) + (red[2] + red[3]));
    out[i] = accumulate ? out[i] + v : v;
  }
}

extern "C" int tpgsr_reduce_partials(const float* part, int Z, int n, float* out, int accumulate, void* stream) {
  TPGSR_CHECK_ARG(part && out && Z > 0 && n > 0, "tpgsr_reduce_partials: bad arguments");
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, part, Z, n, out, accumulate);
  TPGSR_LAUNCH_CHECK("tpgsr_reduce_partials");
}
