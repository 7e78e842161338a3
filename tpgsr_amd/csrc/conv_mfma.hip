// Implicit-GEMM convolution / linear layers on the gfx950 fp32 matrix cores.
//
//   fwd / dgrad :  out[m][n]   = sum_k A[m][k] * wt[k][n]          (tile 64 pixels x 64 channels, 4 waves)
//   wgrad       :  part[k][n]  = sum_m A[m][k] * dy[m][n]          (tile 64 k x 64 channels, split over m)
//
// A[m][k] is never materialised: it is gathered (im2col on the fly, zero padding, optional un-PixelShuffle)
// from the NHWC activation by the tile loader, which also applies the producer's pending per-channel affine
// (train-mode BatchNorm), activation (mish / ReLU) and residual add.  Both kernels stage A as As[k][m] and the
// second operand row-major in LDS; v_mfma_f32_32x32x2_f32 fragments are fetched with conflict-free ds_read_b32
// (lane l reads row k0 + (l>>5), column (l&31)).  fp32 in, fp32 accumulate: bit-for-bit an fmaf chain.
#include "common.h"
#include <mutex>

// 1: all MFMA fragments of a K chunk are read from LDS before its first MFMA (one LDS round trip per chunk, +32 VGPRs:
// 4 waves / SIMD); 0: the compiler interleaves read pairs with the MFMAs (6 waves / SIMD).  Measured on MI355X: equal
// on the 768-tile 64->64 convs (45.0 vs 45.5 us), 0 wins on larger grids (3x3 64->256: 137 vs 152 us) -> default 0.
#ifndef TPGSR_FRAG_PRELOAD
#define TPGSR_FRAG_PRELOAD 0
#endif
#include <utility>
#include <vector>
#include "conv_loader.h"
#include "conv_launch.h"

// ------------------------------------------------------------------------------------------------------
// forward / data-gradient kernel
// ------------------------------------------------------------------------------------------------------
// SPLIT: 1 in every instantiation.  (SPLIT = 2 -- two 256-thread groups per workgroup on the two halves of the K range of the SAME 64x64
// tile, combined through LDS -- measured neutral and is no longer built or dispatched: DESIGN.md "Retired experiments".  The parameter
// stays because taking it out of the text changes the register allocation of two of the ten instantiations.)
template <int LD, int SPLIT>   // LD >= 0: vector quad loader with compile-time prologue bits; LD < 0: generic scalar loader
__global__ __launch_bounds__(256 * SPLIT) void conv_fwd_kernel(tpgsr_conv_args a, int M, int K, int vecB) {
  constexpr bool VEC_A = LD >= 0;
  __shared__ float As_[SPLIT][KC][ALD];
  __shared__ float Bs_[SPLIT][KC][BN];
  const int grp = SPLIT > 1 ? (int)(threadIdx.x >> 8) : 0;
  float (*As)[ALD] = As_[grp];
  float (*Bs)[BN] = Bs_[grp];
  const int tid = threadIdx.x & 255;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int nbn = (a.Cout + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int mblk = tile / nbn;
  const int m0 = mblk * BM, n0 = (tile - mblk * nbn) * BN;
  const int nchunks_all = (K + KC - 1) / KC;
  const int nchunks = (nchunks_all + SPLIT - 1) / SPLIT;   // chunks per group; a group's surplus chunk loads zeros
  const int ch0 = grp * nchunks;

  // A staging: thread -> quad (tid&7) of the chunk, pixels (tid>>3) and (tid>>3)+32
  const int aq = tid & 7;
  const int am0 = tid >> 3;
  PixelPos px0 = decode_pixel(a, m0 + am0, M);
  PixelPos px1 = decode_pixel(a, m0 + am0 + 32, M);
  // B staging: rows (tid>>4) and (tid>>4)+16, columns (tid&15)*4
  const int bk0 = tid >> 4;
  const int bc = (tid & 15) * 4;

  float4 ra0, ra1, rb0, rb1;
  ARaw qa0, qa1;
  float4 qs = make_float4(1.f, 1.f, 1.f, 1.f), qt = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int LDV = LD < 0 ? 0 : LD;
  const int Wr_ = real_w(a);
  const size_t in_floats = a.in_ps ? (size_t)a.N * a.H * a.W * a.Cin : (size_t)a.N * a.H * Wr_ * a.in_ld;
  const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(a.in, in_floats);
  const __amdgpu_buffer_rsrc_t rs_in2 = (LDV & 16) ? make_rsrc(a.in_b, (size_t)a.N * Wr_ * a.in_b_ld)
                                                   : make_rsrc(a.in2 ? a.in2 : a.in, (size_t)a.N * a.H * Wr_ * a.in2_ld);
  const int wld = a.wt_ld > 0 ? a.wt_ld : a.Cout;
  const __amdgpu_buffer_rsrc_t rs_wt = make_rsrc(a.wt, (size_t)K * wld);
  KPos kp = kpos_init(a, VEC_A ? ch0 * (KC / 4) + aq : 0);   // this thread's quad of chunk ch0; load_chunk advances it
  auto load_chunk = [&](int ch) {
    if (VEC_A) {
      qa0 = load_a_raw<LDV>(a, rs_in, rs_in2, px0, kp);
      qa1 = load_a_raw<LDV>(a, rs_in, rs_in2, px1, kp);
      if (LDV & 1) {
        qs = *reinterpret_cast<const float4*>(a.in_scale + kp.c);
        qt = *reinterpret_cast<const float4*>(a.in_shift + kp.c);
      }
      kpos_advance(a, kp, KC);
      int k0 = ch * KC + bk0, k1 = k0 + 16;
      const bool cok = n0 + bc < a.Cout;   // rows k >= K fall outside the buffer: hardware zero fill
      rb0 = buf_load4(rs_wt, cok ? ((unsigned)k0 * (unsigned)wld + (unsigned)(a.wt_coff + n0 + bc)) * 4u : OOB_OFF);
      rb1 = buf_load4(rs_wt, cok ? ((unsigned)k1 * (unsigned)wld + (unsigned)(a.wt_coff + n0 + bc)) * 4u : OOB_OFF);
    } else {
      int k = ch * KC + aq * 4;
      ra0 = make_float4(load_a_scalar(a, px0, k, K), load_a_scalar(a, px0, k + 1, K), load_a_scalar(a, px0, k + 2, K),
                        load_a_scalar(a, px0, k + 3, K));
      ra1 = make_float4(load_a_scalar(a, px1, k, K), load_a_scalar(a, px1, k + 1, K), load_a_scalar(a, px1, k + 2, K),
                        load_a_scalar(a, px1, k + 3, K));
      int k0 = ch * KC + bk0, k1 = k0 + 16;
      rb0 = load_row4(a.wt + a.wt_coff, k0, wld, n0 + bc, a.Cout, k0 < K, vecB);
      rb1 = load_row4(a.wt + a.wt_coff, k1, wld, n0 + bc, a.Cout, k1 < K, vecB);
    }
  };
  auto store_chunk = [&]() {
    if (VEC_A) {
      ra0 = finish_a<LDV>(a, qa0, qs, qt);
      ra1 = finish_a<LDV>(a, qa1, qs, qt);
    }
    As[aq * 4 + 0][am0] = ra0.x;
    As[aq * 4 + 1][am0] = ra0.y;
    As[aq * 4 + 2][am0] = ra0.z;
    As[aq * 4 + 3][am0] = ra0.w;
    As[aq * 4 + 0][am0 + 32] = ra1.x;
    As[aq * 4 + 1][am0 + 32] = ra1.y;
    As[aq * 4 + 2][am0 + 32] = ra1.z;
    As[aq * 4 + 3][am0 + 32] = ra1.w;
    *reinterpret_cast<float4*>(&Bs[bk0][bc]) = rb0;
    *reinterpret_cast<float4*>(&Bs[bk0 + 16][bc]) = rb1;
  };

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  load_chunk(ch0);
  store_chunk();
  __syncthreads();
  const int arow = lane >> 5;
  const int acol = wm * 32 + (lane & 31);
  const int bcol = wn * 32 + (lane & 31);
#ifdef TPGSR_CONV_ABLATE_BUILD   // timing ablations (tools/bench_kernels.py); runtime flags would force the accumulator
  const bool abl_noload = vecB & 256, abl_nolds = vecB & 512, abl_nobar = vecB & 1024;   // through VGPR copies every chunk
#else
  constexpr bool abl_noload = false, abl_nolds = false, abl_nobar = false;
#endif
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch + 1 < nchunks && !abl_noload) load_chunk(ch0 + ch + 1);
    float av[KC / 2], bv[KC / 2];
    if (!abl_nolds) {
#pragma unroll
      for (int kk = 0; kk < KC / 2; ++kk) {   // all fragment reads first: one LDS round trip per chunk, not one per MFMA pair
        av[kk] = As[2 * kk + arow][acol];
        bv[kk] = Bs[2 * kk + arow][bcol];
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < KC / 2; ++kk) av[kk] = As[arow][acol], bv[kk] = Bs[arow][bcol];
    }
#if TPGSR_FRAG_PRELOAD
    __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise sinks each read pair next to its MFMAs again)
#endif
#pragma unroll
    for (int kk = 0; kk < KC / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);   // keep the prologue arithmetic / LDS stores of the next tile behind the MFMAs
    if (!abl_nobar) __syncthreads();
    if (ch + 1 < nchunks) {
      store_chunk();
      if (!abl_nobar) __syncthreads();
    }
  }

  if (SPLIT > 1) {   // combine the two K halves: group 1 parks its accumulators in LDS, group 0 adds them
    float* xch = &As_[0][0][0];   // As_ = 2*KC*ALD = 4160 floats >= the 64x64 tile; nobody reads it after the loop's last barrier
    if (grp == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) xch[(wave * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (grp == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += xch[(wave * 16 + r) * 64 + lane];
    }
    __syncthreads();
  }
  const bool active = grp == 0;   // group 1 keeps running (barriers below stay workgroup-uniform) but writes nothing
  // ---- epilogue: bias, activation, (pixel-shuffled) store, BN partial statistics ----
  const int n = n0 + bcol;
  const bool nvalid = n < a.Cout;
  const float bias = (a.bias && nvalid) ? a.bias[n] : 0.f;
  float s = 0.f, ss = 0.f;
  const int ohw = a.OH * a.OW;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    int m = m0 + wm * 32 + row;
    if (m < M && nvalid && active) {
      float raw = acc[r];
      s += raw;
      ss += raw * raw;
      float v = apply_act(raw + bias, a.out_act);
      if (!a.out_ps) {
        a.out[(size_t)m * a.out_ld + a.out_coff + n] = v;
      } else {
        int nn = m / ohw;
        int rem = m - nn * ohw;
        int oh = rem / a.OW, ow = rem - oh * a.OW;
        int cs = n >> 2, i = (n >> 1) & 1, j = n & 1;
        a.out[((size_t)(nn * 2 * a.OH + 2 * oh + i) * (2 * a.OW) + 2 * ow + j) * (a.Cout >> 2) + cs] = v;
      }
    }
  }
  if (a.bn_partial) {
    s += __shfl_xor(s, 32);
    ss += __shfl_xor(ss, 32);
    float* red = &Bs[0][0];  // group-private; all MFMA reads finished behind the loop's final barrier
    if (lane < 32) {
      red[(wm * 2 + 0) * BN + bcol] = s;
      red[(wm * 2 + 1) * BN + bcol] = ss;
    }
    __syncthreads();
    if (active && tid < BN && n0 + tid < a.Cout) {
      float* dst = a.bn_partial + (size_t)mblk * 2 * a.Cout;
      dst[n0 + tid] = red[0 * BN + tid] + red[2 * BN + tid];
      dst[a.Cout + n0 + tid] = red[1 * BN + tid] + red[3 * BN + tid];
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Weights-stationary 3x3 conv for the 64-channel trunk (RRB conv1/conv2, conv7 and their data gradients: Cin = Cout = 64,
// pad 1, image width 64 = one 64-pixel tile per image row, plain loader).  One 12-wave workgroup owns three image rows:
// the 3 x 3 x 32 x 64 weight slice of a 32-channel pass (72 KB) is brought into LDS once by LDS-DMA and shared by the
// three 4-wave groups, each group brings the 3 x 66-pixel halo of its row (25 KB, zero page for padding); then 9 taps x
// 16 MFMAs per wave run out of LDS with no barrier in between.  Global traffic 76 MB instead of 226 MB for the C2 shape;
// 37.5 us vs 45 us for the im2col tile loop (tools/lab/conv_glds_lab.hip).
//   LDS images: halo [pixel][8 quads], quad position q ^ ((pixel >> 1) & 7) (source-side swizzle: the LDS side of an LDS-DMA
//   is lane-linear) -> conflict-free ds_read_b128 A fragments; weights [tap][32][64] row-major -> conflict-free b32.
//   K index of MFMA j for lane half h: 4 * (2 * (j >> 2) + h) + (j & 3) within the 32-channel slice.
// ------------------------------------------------------------------------------------------------------
#define WS_HP (3 * 66)
#define WS_HPAD ((WS_HP + 7) / 8 * 8)
#define WS_LDS_FLOATS (9 * 32 * 64 + 3 * WS_HPAD * 32)
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
__device__ __forceinline__ void glds16(const float* src, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)lds_wave_base, 16, 0, 0);
}

__global__ __launch_bounds__(768) void conv3x3_wstat_kernel(tpgsr_conv_args a, const float* __restrict__ zero, int M) {
  extern __shared__ __attribute__((aligned(16))) float ws_smem[];
  float* Ws = ws_smem;                          // [9][32][64]
  const int tid = threadIdx.x, L = tid & 63, wv = tid >> 6;
  const int grp = wv >> 2, w = wv & 3;
  const int wm = w & 1, wn = w >> 1;
  const int H = a.H, W = 64;
  const int row = blockIdx.x * 3 + grp;         // image row (n * H + oh) = 64-pixel tile index
  const int m0 = row * 64;
  const bool rowok = m0 < M;
  const int n = rowok ? row / H : 0, oh = rowok ? row - n * H : 0;
  float* Hs = ws_smem + 9 * 32 * 64 + grp * WS_HPAD * 32;
  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int am = wm * 32 + (L & 31), h = L >> 5;
  const int bn = wn * 32 + (L & 31);
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    for (int g = wv; g < 72; g += 12) {         // weight rows tap*64 + pass*32 + r -> Ws[tap][r][:], 4 rows per LDS-DMA
      int rr = g * 4 + (L >> 4);
      int tap = rr >> 5, r = rr & 31;
      glds16(a.wt + (size_t)(tap * 64 + pass * 32 + r) * 64 + (L & 15) * 4, &Ws[g * 4 * 64]);
    }
    for (int g = w; g < WS_HPAD / 8; g += 4) {  // this group's halo, 8 pixels per LDS-DMA
      int P = g * 8 + (L >> 3);
      int r = P / 66, cc = P - r * 66;
      int ih = oh - 1 + r, iw = cc - 1;
      bool ok = rowok && P < WS_HP && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
      int q = (L & 7) ^ ((P >> 1) & 7);
      const float* src = ok ? a.in + ((size_t)(n * H + ih) * W + iw) * a.in_ld + a.in_coff + pass * 32 + q * 4 : zero + (L & 7) * 4;
      glds16(src, &Hs[g * 8 * 32]);
    }
    __syncthreads();                            // drains the LDS-DMAs (vmcnt(0)) of every wave
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - kh * 3;
      const int P = kh * 66 + am + kw;
      const float* Wt = Ws + tap * 32 * 64;
      float4 a4[4];
      float b[16];
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        int pos = (2 * qi + h) ^ ((P >> 1) & 7);
        a4[qi] = *reinterpret_cast<const float4*>(&Hs[P * 32 + pos * 4]);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = Wt[(4 * (2 * (j >> 2) + h) + (j & 3)) * 64 + bn];
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[qi].x, b[4 * qi + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[qi].y, b[4 * qi + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[qi].z, b[4 * qi + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[qi].w, b[4 * qi + 3], acc, 0, 0, 0);
      }
    }
  }
  // ---- epilogue: bias, store, BN partial statistics (one 64-pixel row block per group, as conv_fwd_kernel) ----
  const float bias = a.bias ? a.bias[bn] : 0.f;
  float s = 0.f, ss = 0.f;
  if (rowok) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int rw = (r & 3) + 8 * (r >> 2) + 4 * (L >> 5);
      int m = m0 + wm * 32 + rw;
      float raw = acc[r];
      s += raw;
      ss += raw * raw;
      a.out[(size_t)m * a.out_ld + a.out_coff + bn] = raw + bias;
    }
  }
  if (a.bn_partial) {
    __syncthreads();                            // all groups are done reading their halos: reuse them as reduction scratch
    s += __shfl_xor(s, 32);
    ss += __shfl_xor(ss, 32);
    float* red = Hs;                            // [wm][2][64]
    if (L < 32) {
      red[(wm * 2 + 0) * 64 + bn] = s;
      red[(wm * 2 + 1) * 64 + bn] = ss;
    }
    __syncthreads();
    const int t = tid & 255;
    if (rowok && t < 64) {
      float* dst = a.bn_partial + (size_t)row * 2 * 64;
      dst[t] = red[0 * 64 + t] + red[2 * 64 + t];
      dst[64 + t] = red[1 * 64 + t] + red[3 * 64 + t];
    }
  }
}

static_assert(sizeof(float) * WS_LDS_FLOATS == kWstatLdsBytes, "conv_route.h sizes the weights-stationary kernel's LDS");

int unsupported_ld(const char* who, int ld) {
  tpgsr_set_error("%s: unsupported loader combination %d", who, ld);
  return TPGSR_ERR_ARG;
}

// opt-in to > 64 KB of dynamic LDS, per (kernel, device): raised to the largest size seen so far
int lds_opt_in(const void* fn, size_t bytes, const char* who) {
  if (bytes <= 64 * 1024) return 0;
  static std::mutex mu;
  static std::vector<std::pair<std::pair<const void*, int>, size_t>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    tpgsr_set_error("%s: hipGetDevice failed", who);
    return TPGSR_ERR_LAUNCH;
  }
  std::lock_guard<std::mutex> lock(mu);
  size_t* cur = nullptr;
  for (auto& d : done)
    if (d.first.first == fn && d.first.second == dev) cur = &d.second;
  if (!cur || *cur < bytes) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
      tpgsr_set_error("%s: LDS opt-in (%zu bytes) failed", who, bytes);
      return TPGSR_ERR_LAUNCH;
    }
    if (cur) *cur = bytes; else done.push_back({{fn, dev}, bytes});
  }
  return 0;
}

static int check_conv_args(const tpgsr_conv_args* a, const char* who) {
  TPGSR_CHECK_ARG(a && a->in, "%s: null input", who);
  TPGSR_CHECK_ARG(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0 && a->KH > 0 && a->KW > 0,
                  "%s: non-positive dimension", who);
  TPGSR_CHECK_ARG(a->OH > 0 && a->OW > 0, "%s: non-positive output size", who);
  TPGSR_CHECK_ARG(a->in_ld >= (a->in_b ? a->cin_a : a->Cin) + a->in_coff || a->in_ps, "%s: in_ld %d < Cin %d + coff %d", who,
                  a->in_ld, a->Cin, a->in_coff);
  if (a->in_b)
    TPGSR_CHECK_ARG(a->cin_a > 0 && a->cin_a < a->Cin && (a->cin_a & 3) == 0 && a->in_b_ld >= a->Cin - a->cin_a && !a->in_ps &&
                    !a->in2 && ((a->Cin & 3) || (a->in_b_ld & 3) == 0), "%s: bad concat description", who);
  if (a->in_dil_w > 1) TPGSR_CHECK_ARG((a->W - 1) % a->in_dil_w == 0 && !a->in_ps, "%s: bad input dilation", who);
  if (a->in_ps) TPGSR_CHECK_ARG((a->Cin & 3) == 0 && a->in_coff == 0, "%s: in_ps needs Cin %% 4 == 0", who);
  if ((a->Cin & 3) == 0 && !a->in_ps)
    TPGSR_CHECK_ARG((a->in_ld & 3) == 0 && (a->in_coff & 3) == 0 && ((uintptr_t)a->in & 15) == 0,
                    "%s: vector loader needs 16-byte aligned rows", who);
  if (a->in2) TPGSR_CHECK_ARG(a->in2_ld >= a->Cin && ((a->Cin & 3) || (a->in2_ld & 3) == 0), "%s: bad in2_ld", who);
  TPGSR_CHECK_ARG((a->in_scale == nullptr) == (a->in_shift == nullptr), "%s: in_scale/in_shift must come together", who);
  TPGSR_CHECK_ARG(!a->in2_scale || (a->in2 && a->in_scale && !a->in_act && !a->in_b && !a->in_ps && (((uintptr_t)a->in2_scale) & 15) == 0),
                  "%s: in2_scale goes with in2 + in_scale / in_shift and nothing else (a = in * s + t + in2 * s2)", who);
  // the loaders address their operands through buffer resources: 32-bit byte offsets inside a 2 GiB window (make_rsrc).  Fail
  // loudly instead of reading zeros past it (one operand of bs x 64 channels x 32x128 reaches 2 GiB at bs = 2048).
  const long long pix = (long long)a->N * a->H * a->W, win = 0x7fffffffll;
  TPGSR_CHECK_ARG(pix * (a->in_ps ? a->Cin : a->in_ld) * 4 <= win, "%s: input operand exceeds the 2 GiB buffer-addressing window (%lld pixels x %d)",
                  who, pix, a->in_ps ? a->Cin : a->in_ld);
  if (a->in2) TPGSR_CHECK_ARG(pix * a->in2_ld * 4 <= win, "%s: second input operand exceeds the 2 GiB buffer-addressing window", who);
  return 0;
}

extern "C" int tpgsr_conv_fwd(const tpgsr_conv_args* a, void* stream) {
  int rc = check_conv_args(a, "tpgsr_conv_fwd");
  if (rc) return rc;
  TPGSR_CHECK_ARG(a->wt && a->out, "tpgsr_conv_fwd: null weight/output");
  TPGSR_CHECK_ARG(a->out_ps || a->out_ld >= a->Cout + a->out_coff, "tpgsr_conv_fwd: out_ld too small");
  if (a->out_ps) TPGSR_CHECK_ARG((a->Cout & 3) == 0, "tpgsr_conv_fwd: out_ps needs Cout %% 4 == 0");
  TPGSR_CHECK_ARG(a->out_act == TPGSR_ACT_NONE || a->out_act == TPGSR_ACT_RELU || a->out_act == TPGSR_ACT_TANH,
                  "tpgsr_conv_fwd: unsupported out_act %d", a->out_act);
  long long M = (long long)a->N * a->OH * a->OW;
  int K = a->KH * a->KW * a->Cin;
  TPGSR_CHECK_ARG(M < (1ll << 31), "tpgsr_conv_fwd: M too large");
  hipStream_t st = (hipStream_t)stream;
  if (a->bnb_y) {   // BatchNorm-backward statistics / activation backward in the epilogue
    TPGSR_CHECK_ARG(!a->out_ps && !a->bias && a->out_act == TPGSR_ACT_NONE,
                    "tpgsr_conv_fwd: bnb_y goes with a plain dense data-gradient store (no bias, no output activation, no pixel shuffle)");
    TPGSR_CHECK_ARG(a->bnb_act == TPGSR_ACT_NONE || a->bnb_act == TPGSR_ACT_RELU || a->bnb_act == TPGSR_ACT_MISH, "tpgsr_conv_fwd: bnb_act %d", a->bnb_act);
    TPGSR_CHECK_ARG((a->bnb_scale == nullptr) == (a->bnb_shift == nullptr), "tpgsr_conv_fwd: bnb_scale / bnb_shift must come together");
    if (a->bn_partial)
      TPGSR_CHECK_ARG(a->bnb_mean && a->bnb_rstd && (a->bnb_act == TPGSR_ACT_NONE || a->bnb_scale),
                      "tpgsr_conv_fwd: BatchNorm-backward sums need bnb_mean, bnb_rstd (and bnb_scale / bnb_shift under an activation)");
    else
      TPGSR_CHECK_ARG(a->bnb_store_dz, "tpgsr_conv_fwd: bnb_y without bn_partial and without bnb_store_dz does nothing");
  }
  const bool xbf = xbf_eligible(a);   // bf16 matrix cores with split operands: vector loader + pre-split weights required
  if (xbf) {
    TPGSR_CHECK_ARG(a->terms >= 1 && a->terms <= 3, "tpgsr_conv_fwd: terms must be 0, 1, 2 or 3");
    TPGSR_CHECK_ARG(a->kp >= K && (a->kp & 31) == 0 && ((uintptr_t)a->wt_bf & 15) == 0, "tpgsr_conv_fwd: bad split operand (kp %d, K %d)", a->kp, K);
    TPGSR_CHECK_ARG(a->wt_bf_cin == 0 || (a->wt_bf_cin == a->Cin && (a->Cin & 31) == 0),
                    "tpgsr_conv_fwd: weights were split in channel-block order for Cin %d, the convolution has Cin %d", a->wt_bf_cin, a->Cin);
  } else {
    TPGSR_CHECK_ARG(a->bn_row_tiles <= 1, "tpgsr_conv_fwd: bn_row_tiles %d needs the whole-CU halo kernel (split-bf16 path)", a->bn_row_tiles);
    TPGSR_CHECK_ARG(!a->bnb_y, "tpgsr_conv_fwd: the BatchNorm-backward epilogue (bnb_y) exists in the split-bf16 kernels only (terms > 0, wt_bf, Cin %% 4 == 0)");
  }
  const tpgsr_conv_route_t r = conv_fwd_route(a, M);
  if (xbf && a->sk_splits <= 1 && r.kernel != TPGSR_CONV_XBF_HALO3) {      // (an explicit split count never reached these two checks)
    TPGSR_CHECK_ARG(!(r.ld & 32), "tpgsr_conv_fwd: a scaled residual operand (in2_scale) exists in the whole-CU halo kernel's loader only, which does not "
                    "take this launch (ask tpgsr_conv_in2_scale_ok first)");
    TPGSR_CHECK_ARG(a->bn_row_tiles <= 1, "tpgsr_conv_fwd: bn_row_tiles %d is the whole-CU halo kernel's, which does not take this launch "
                    "(ask tpgsr_conv_bn_row_tiles first)", a->bn_row_tiles);
  }
  dim3 grid(cdiv(M, BM) * cdiv(a->Cout, BN));
  switch (r.kernel) {
    case TPGSR_CONV_XBF_SPLITK:
    case TPGSR_CONV_XBF_TILE: return conv_fwd_xbf_launch(a, M, K, r, st);
    case TPGSR_CONV_XBF_HALO3: return conv_halo3_xbf_launch(a, M, r, st);
    case TPGSR_CONV_XBF_HALO: return conv_halo_xbf_launch(a, M, r, st);
    case TPGSR_CONV_XBF_PANEL: return conv_panel_xbf_launch(a, M, r, st);
    case TPGSR_CONV_F32_WSTAT: {   // the 64-channel 3x3 trunk convs on 64-wide maps (TPGSR_CONV_WSTAT=0 falls back to the tile loop)
      // per device, set up once under a lock: 256 B of zeros (source of the halo's padding pixels; zeroed on the launch
      // stream and waited for, so every later launch on any stream sees it)
      static float* zero_page[64] = {nullptr};
      static std::mutex init_mu;
      int dev = 0;
      if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        tpgsr_set_error("tpgsr_conv_fwd: hipGetDevice failed");
        return TPGSR_ERR_LAUNCH;
      }
      {
        std::lock_guard<std::mutex> lock(init_mu);
        if (!zero_page[dev]) {
          hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
          if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            tpgsr_set_error("tpgsr_conv_fwd: first use of the weights-stationary conv on device %d happens inside a stream capture; "
                            "run one eager step before capturing", dev);
            return TPGSR_ERR_LAUNCH;
          }
          float* zp = nullptr;
          if (hipMalloc((void**)&zp, 256) != hipSuccess || hipMemsetAsync(zp, 0, 256, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            tpgsr_set_error("tpgsr_conv_fwd: zero page set-up failed");
            return TPGSR_ERR_LAUNCH;
          }
          zero_page[dev] = zp;
        }
      }
      rc = lds_opt_in((const void*)conv3x3_wstat_kernel, r.lds_bytes, "tpgsr_conv_fwd(weights-stationary)");
      if (rc) return rc;
      const int rows = (int)(M / 64);
      hipLaunchKernelGGL(conv3x3_wstat_kernel, dim3((rows + 2) / 3), dim3(768), r.lds_bytes, st, *a, zero_page[dev], (int)M);
      break;
    }
    case TPGSR_CONV_F32_SCALAR: {
      const int wld = a->wt_ld > 0 ? a->wt_ld : a->Cout;
      const int vecB = ((wld & 3) == 0 && ((uintptr_t)a->wt & 15) == 0 && (a->wt_coff & 3) == 0) ? 1 : 0;   // rows padded to a multiple of 4 floats
      hipLaunchKernelGGL((conv_fwd_kernel<-1, 1>), grid, dim3(256), 0, st, *a, (int)M, K, vecB);
      break;
    }
    case TPGSR_CONV_F32_TILE:
#define TPGSR_FWD_CASE(B) case B: hipLaunchKernelGGL((conv_fwd_kernel<B, 1>), grid, dim3(256), 0, st, *a, (int)M, K, 1); break;
      switch (r.ld) {
        TPGSR_FWD_CASE(0) TPGSR_FWD_CASE(1) TPGSR_FWD_CASE(3) TPGSR_FWD_CASE(4) TPGSR_FWD_CASE(5) TPGSR_FWD_CASE(7)
        TPGSR_FWD_CASE(8) TPGSR_FWD_CASE(2) TPGSR_FWD_CASE(17)
        default: return unsupported_ld("tpgsr_conv_fwd", r.ld);
      }
#undef TPGSR_FWD_CASE
      break;
    default: return unsupported_ld("tpgsr_conv_fwd", r.ld);
  }
  TPGSR_LAUNCH_CHECK("tpgsr_conv_fwd");
}

// ------------------------------------------------------------------------------------------------------
// weight-gradient kernel:  part[z][k][n] = sum_{m in split z} A[m][k] * dy[m][n]
// ------------------------------------------------------------------------------------------------------
#define WK 64  // k rows per block
#define WM 32  // pixels per staged chunk
#define WALD (WM + 1)
static_assert(KC == kConvKC && BN == kConvBN && WK == kWgradWK && WM == kWgradWM, "conv_route.h plans splits over these tiles");

__device__ __forceinline__ float4 load_dy4(const tpgsr_wgrad_args& w, const PixelPos& p, int m, int col, int vec) {
  const tpgsr_conv_args& a = w.c;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!w.dy_ps) return load_row4(w.dy + w.dy_coff, (size_t)m, w.dy_ld, col, a.Cout, p.valid, vec);
  if (!p.valid || col >= a.Cout) return v;
  // logical channels col..col+3 = (cs = col/4, i, j) of a [N][2OH][2OW][Cout/4] tensor
  int C4 = a.Cout >> 2, cs = col >> 2;
  size_t W2 = 2 * (size_t)a.OW;
  const float* b = w.dy + ((size_t)(p.n * 2 * a.OH + 2 * p.oh) * W2 + 2 * p.ow) * C4 + cs;
  v.x = b[0];
  v.y = b[C4];
  v.z = b[W2 * C4];
  v.w = b[W2 * C4 + C4];
  return v;
}

template <int LD>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(tpgsr_wgrad_args w, int M, int K, int MB, int vecY) {
  constexpr bool VEC_A = LD >= 0;
  __shared__ float As[WK][WALD];
  __shared__ float Ys[WM][BN];
  const tpgsr_conv_args& a = w.c;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wk = wave & 1, wn = wave >> 1;
  const int nkb = (K + WK - 1) / WK, nnb = (a.Cout + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);       // k-block fastest: the k-blocks of one pixel split share an L2
  const int kblk = tile % nkb, nblk = (tile / nkb) % nnb, zblk = tile / (nkb * nnb);
  const int k0 = kblk * WK, n0 = nblk * BN;
  const int mbeg = zblk * MB;
  const int mend = min(M, mbeg + MB);

  // A staging: quad (tid&15) of this block's 64 k rows (fixed for the whole kernel), pixels (tid>>4), +16
  const int aq = tid & 15;
  const int ap0 = tid >> 4;
  const KPos kp = kpos_init(a, VEC_A ? (k0 >> 2) + aq : 0);
  const int ac = kp.c;
  const int yr0 = tid >> 4;
  const int yc = (tid & 15) * 4;

  float4 ra0, ra1, ry0, ry1;
  ARaw qa0, qa1;
  float4 qs = make_float4(1.f, 1.f, 1.f, 1.f), qt = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int LDV = LD < 0 ? 0 : LD;
  const int Wr_ = real_w(a);
  const size_t in_floats = a.in_ps ? (size_t)a.N * a.H * a.W * a.Cin : (size_t)a.N * a.H * Wr_ * a.in_ld;
  const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(a.in, in_floats);
  const __amdgpu_buffer_rsrc_t rs_in2 = (LDV & 16) ? make_rsrc(a.in_b, (size_t)a.N * Wr_ * a.in_b_ld)
                                                   : make_rsrc(a.in2 ? a.in2 : a.in, (size_t)a.N * a.H * Wr_ * a.in2_ld);
  const __amdgpu_buffer_rsrc_t rs_dy = make_rsrc(w.dy, w.dy_ps ? (size_t)M * a.Cout : (size_t)M * w.dy_ld);
  if (VEC_A && (LDV & 1)) {
    qs = *reinterpret_cast<const float4*>(a.in_scale + ac);
    qt = *reinterpret_cast<const float4*>(a.in_shift + ac);
  }
  auto load_chunk = [&](int mc) {
    int ma = mc + ap0, mb = mc + ap0 + 16;
    PixelPos p0 = decode_pixel(a, ma, mend);
    PixelPos p1 = decode_pixel(a, mb, mend);
    if (VEC_A) {
      qa0 = load_a_raw<LDV>(a, rs_in, rs_in2, p0, kp);
      qa1 = load_a_raw<LDV>(a, rs_in, rs_in2, p1, kp);
      if (!w.dy_ps) {
        const bool cok = n0 + yc < a.Cout;
        ry0 = buf_load4(rs_dy, (p0.valid && cok) ? ((unsigned)ma * (unsigned)w.dy_ld + (unsigned)(w.dy_coff + n0 + yc)) * 4u : OOB_OFF);
        ry1 = buf_load4(rs_dy, (p1.valid && cok) ? ((unsigned)mb * (unsigned)w.dy_ld + (unsigned)(w.dy_coff + n0 + yc)) * 4u : OOB_OFF);
      } else {
        ry0 = load_dy4(w, p0, ma, n0 + yc, 1);
        ry1 = load_dy4(w, p1, mb, n0 + yc, 1);
      }
    } else {
      int k = k0 + aq * 4;
      ra0 = make_float4(load_a_scalar(a, p0, k, K), load_a_scalar(a, p0, k + 1, K), load_a_scalar(a, p0, k + 2, K),
                        load_a_scalar(a, p0, k + 3, K));
      ra1 = make_float4(load_a_scalar(a, p1, k, K), load_a_scalar(a, p1, k + 1, K), load_a_scalar(a, p1, k + 2, K),
                        load_a_scalar(a, p1, k + 3, K));
      ry0 = load_dy4(w, p0, ma, n0 + yc, vecY);
      ry1 = load_dy4(w, p1, mb, n0 + yc, vecY);
    }
  };
  auto store_chunk = [&]() {
    if (VEC_A) {
      ra0 = finish_a<LDV>(a, qa0, qs, qt);
      ra1 = finish_a<LDV>(a, qa1, qs, qt);
    }
    As[aq * 4 + 0][ap0] = ra0.x;
    As[aq * 4 + 1][ap0] = ra0.y;
    As[aq * 4 + 2][ap0] = ra0.z;
    As[aq * 4 + 3][ap0] = ra0.w;
    As[aq * 4 + 0][ap0 + 16] = ra1.x;
    As[aq * 4 + 1][ap0 + 16] = ra1.y;
    As[aq * 4 + 2][ap0 + 16] = ra1.z;
    As[aq * 4 + 3][ap0 + 16] = ra1.w;
    *reinterpret_cast<float4*>(&Ys[yr0][yc]) = ry0;
    *reinterpret_cast<float4*>(&Ys[yr0 + 16][yc]) = ry1;
  };

  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float dbacc = 0.f;
  const bool want_db = (w.dbpart != nullptr) && kblk == 0 && tid < BN;

  if (mbeg < mend) {
    load_chunk(mbeg);
    store_chunk();
  }
  __syncthreads();
  const int arow = wk * 32 + (lane & 31);
  const int bcol = wn * 32 + (lane & 31);
  const int half = lane >> 5;
  for (int mc = mbeg; mc < mend; mc += WM) {
    const bool more = mc + WM < mend;
    if (more) load_chunk(mc + WM);
    float av[WM / 2], bv[WM / 2];
#pragma unroll
    for (int mm = 0; mm < WM / 2; ++mm) {
      av[mm] = As[arow][2 * mm + half];
      bv[mm] = Ys[2 * mm + half][bcol];
    }
#if TPGSR_FRAG_PRELOAD
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int mm = 0; mm < WM / 2; ++mm) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mm], bv[mm], acc, 0, 0, 0);
    if (want_db) {
#pragma unroll 8
      for (int r = 0; r < WM; ++r) dbacc += Ys[r][tid];
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }
  const int n = n0 + bcol;
  float* dst = w.part + (size_t)zblk * K * a.Cout;
  if (n < a.Cout) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int k = k0 + wk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (k < K) dst[(size_t)k * a.Cout + n] = acc[r];
    }
  }
  if (want_db && n0 + tid < a.Cout) w.dbpart[(size_t)zblk * a.Cout + n0 + tid] = dbacc;
}

extern "C" int tpgsr_conv_wgrad(const tpgsr_wgrad_args* w, void* stream) {
  TPGSR_CHECK_ARG(w != nullptr, "tpgsr_conv_wgrad: null args");
  int rc = check_conv_args(&w->c, "tpgsr_conv_wgrad");
  if (rc) return rc;
  TPGSR_CHECK_ARG(w->dy && w->part, "tpgsr_conv_wgrad: null dy/part");
  const tpgsr_conv_args* a = &w->c;
  if (w->dy_ps) TPGSR_CHECK_ARG((a->Cout & 3) == 0 && w->dy_coff == 0, "tpgsr_conv_wgrad: dy_ps needs Cout %% 4 == 0");
  else TPGSR_CHECK_ARG(w->dy_ld >= a->Cout + w->dy_coff, "tpgsr_conv_wgrad: dy_ld too small");
  long long M = (long long)a->N * a->OH * a->OW;
  int K = a->KH * a->KW * a->Cin;
  TPGSR_CHECK_ARG(M < (1ll << 31) && M * (w->dy_ps ? a->Cout : w->dy_ld) * 4 <= 0x7fffffffll,
                  "tpgsr_conv_wgrad: dy exceeds the 2 GiB buffer-addressing window (M %lld)", M);
  hipStream_t st = (hipStream_t)stream;
  const tpgsr_wgrad_route_t r = conv_wgrad_route(w, M);
  if (a->terms > 0 && (a->Cin & 3) == 0 && (r.vecY || w->dy_ps))   // the split-bf16 kernels
    TPGSR_CHECK_ARG(a->terms >= 1 && a->terms <= 3, "tpgsr_conv_wgrad: terms must be 0, 1, 2 or 3");
  dim3 grid(cdiv(K, WK) * cdiv(a->Cout, BN) * r.Z);
  switch (r.kernel) {
    case TPGSR_WGRAD_XBF_HALO: return conv_wgrad_halo_launch(w, M, r, st);
    case TPGSR_WGRAD_XBF_3K:
    case TPGSR_WGRAD_XBF_TILE: return conv_wgrad_xbf_launch(w, M, K, r, st);
    case TPGSR_WGRAD_F32_SCALAR: hipLaunchKernelGGL(conv_wgrad_kernel<-1>, grid, dim3(256), 0, st, *w, (int)M, K, r.MB, r.vecY); break;
    case TPGSR_WGRAD_F32_TILE:
#define TPGSR_WG_CASE(B) case B: hipLaunchKernelGGL(conv_wgrad_kernel<B>, grid, dim3(256), 0, st, *w, (int)M, K, r.MB, r.vecY); break;
      switch (r.ld) {
        TPGSR_WG_CASE(0) TPGSR_WG_CASE(1) TPGSR_WG_CASE(3) TPGSR_WG_CASE(4) TPGSR_WG_CASE(5) TPGSR_WG_CASE(7) TPGSR_WG_CASE(2) TPGSR_WG_CASE(17)
        default: return unsupported_ld("tpgsr_conv_wgrad", r.ld);
      }
#undef TPGSR_WG_CASE
      break;
    default: return unsupported_ld("tpgsr_conv_wgrad", r.ld);
  }
  TPGSR_LAUNCH_CHECK("tpgsr_conv_wgrad");
}

// dw (+)= sum_z part[z][k][co], scattered into the PyTorch layout.  256 threads = 32 outputs x 8 z-lanes: the Z partial
// slabs are summed by 8 lanes in parallel (independent, unrolled loads) and combined through LDS in a fixed order.
__device__ __forceinline__ size_t wgrad_out_index(int tap, int ci, int co, int Cin, int Cout, int KH, int KW, int layout) {
  int kh = tap / KW, kw = tap - kh * KW;
  if (layout == 0) return (((size_t)co * Cin + ci) * KH + kh) * KW + kw;
  if (layout == 1)  // ConvTranspose2d weight wT[ci][co][KH-1-kh][KW-1-kw] == equivalent-conv w_eq[co][ci][kh][kw]
    return (((size_t)ci * Cout + co) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw);
  if (layout == 3)  // InfoGen strip: 1x3 conv tap kw' of the dilated strip == wT[ci][co][1][2 - kw']
    return (((size_t)ci * Cout + co) * 3 + 1) * 3 + (KW - 1 - kw);
  // layout 2: folded tail conv (KH = KS, KW = 1, Cout = KS*Co, n' = kw*Co + co) -> w[co][ci][kh][kw]
  int Co = Cout / KH;
  int tkw = co / Co, tco = co - tkw * Co;
  return (((size_t)tco * Cin + ci) * KH + kh) * KH + tkw;
}

// Slab reduce.  What bounds it is not the 0.57 GB of slabs a C3 step reads but the WRITE side: slabs are [k = (tap, ci)][co] with co
// contiguous, a PyTorch weight is [co][ci][tap] -- written entry by entry that is one read-modify-write of a 4-byte word per output, each
// on a cache line of its own (47 MB of gradients cost the three reduces of a step 360 us at 1.6 TB/s; a version with fully coalesced
// 16-byte slab loads and the same scattered writes took exactly as long).  For `layout` 0 (every convolution and linear layer) a
// workgroup therefore owns a 2-D tile -- ALL taps of CB input channels x 32 output channels, CB = 32 / taps rounded to >= 1 --
// sums it over the slabs (four z-lanes = the four waves, 128 contiguous bytes per row), combines the lanes through LDS in wave order
// and writes it TRANSPOSED: per output channel a contiguous run of CB * taps floats.  Other layouts (transposed convolutions of InfoGen,
// the folded tail) and the bias entries take the linear path: 256 consecutive entries per workgroup.  Deterministic: the order of the
// additions depends on (Z, entry) only.
#define WR_BLK 256
#define WR_MAXR 32          // rows of a tile held in LDS (taps * CB <= 32: the two 9x9 layers take the linear path)
#define WR_PITCH 33         // floats per tile row in LDS: phase 2 walks a column
__host__ __device__ __forceinline__ int wr_cb(int taps) { return taps >= 32 ? 1 : 32 / taps; }
__host__ __device__ __forceinline__ bool wr_tiled(int Cin, int Cout, int KH, int KW, int layout) {
  return layout == 0 && KH * KW * wr_cb(KH * KW) <= WR_MAXR && (Cout & 3) == 0;
}
__host__ __device__ __forceinline__ int wr_weight_blocks(int K, int Cin, int Cout, int KH, int KW, int layout) {
  if (wr_tiled(Cin, Cout, KH, KW, layout)) {
    const int cb = wr_cb(KH * KW);
    return ((Cin + cb - 1) / cb) * ((Cout + 31) / 32);
  }
  return (int)(((size_t)K * Cout + WR_BLK - 1) / WR_BLK);
}

__device__ __forceinline__ void wgrad_reduce_body(float* red /* [4][WR_MAXR * WR_PITCH + 4] */, const float* __restrict__ part,
                                                  const float* __restrict__ dbpart, int Z, int K, int Cin, int Cout, int KH,
                                                  int KW, int layout, float* dw, float* db, int accumulate, float gscale,
                                                  unsigned blk, int cin_ld) {
  if (cin_ld <= 0) cin_ld = Cin;   // k = tap * cin_ld + ci; rows with ci >= Cin or tap >= KH*KW belong to a zero-padded operand
  const size_t total = (size_t)K * Cout;
  const int nwblk = wr_weight_blocks(K, Cin, Cout, KH, KW, layout);
  const int lane = threadIdx.x & 63, zl = threadIdx.x >> 6;
  constexpr int LZ = WR_MAXR * WR_PITCH + 4;       // floats per z-lane in `red`
  if ((int)blk < nwblk && wr_tiled(Cin, Cout, KH, KW, layout)) {
    const int taps = KH * KW, cb = wr_cb(taps), R = taps * cb;
    const int nct = (Cout + 31) / 32;
    const int rt = (int)blk / nct, ct = (int)blk - rt * nct;
    const int c0 = rt * cb, co0 = ct * 32;
    // phase 1: this wave's z-lane of the tile, rows r = tap * cb + c, 8 quads per row: 8 rows per load instruction
    const int quad = lane & 7;
    const bool colok = co0 + quad * 4 < Cout;
    for (int rb = 0; rb < R; rb += 8) {
      const int r = rb + (lane >> 3);
      const int tap = r / cb, c = r - tap * cb;
      const bool ok = r < R && c0 + c < Cin && colok;
      float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
      if (ok) {
        const float* src = part + ((size_t)tap * cin_ld + c0 + c) * Cout + co0 + quad * 4;
        int z = zl;
        for (; z + 12 < Z; z += 16) {          // four independent 16-byte loads in flight
          const float4 v0 = *reinterpret_cast<const float4*>(src + (size_t)z * total);
          const float4 v1 = *reinterpret_cast<const float4*>(src + (size_t)(z + 4) * total);
          const float4 v2 = *reinterpret_cast<const float4*>(src + (size_t)(z + 8) * total);
          const float4 v3 = *reinterpret_cast<const float4*>(src + (size_t)(z + 12) * total);
          s0.x += v0.x; s0.y += v0.y; s0.z += v0.z; s0.w += v0.w;
          s1.x += v1.x; s1.y += v1.y; s1.z += v1.z; s1.w += v1.w;
          s0.x += v2.x; s0.y += v2.y; s0.z += v2.z; s0.w += v2.w;
          s1.x += v3.x; s1.y += v3.y; s1.z += v3.z; s1.w += v3.w;
        }
        for (; z < Z; z += 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (size_t)z * total);
          s0.x += v.x; s0.y += v.y; s0.z += v.z; s0.w += v.w;
        }
      }
      if (r < R) {
        float* d = red + zl * LZ + r * WR_PITCH + quad * 4;
        d[0] = s0.x + s1.x; d[1] = s0.y + s1.y; d[2] = s0.z + s1.z; d[3] = s0.w + s1.w;
      }
    }
    __syncthreads();
    // phase 2: transposed write -- entry e = (local co, j = c * taps + tap): runs of cb * taps contiguous floats per output channel
    for (int e = threadIdx.x; e < 32 * R; e += 256) {
      const int col = e / R, jj = e - col * R;
      const int c = jj / taps, tap = jj - c * taps;
      if (co0 + col < Cout && c0 + c < Cin) {
        const int r = tap * cb + c;
        const int a = r * WR_PITCH + col;
        float v = ((red[a] + red[LZ + a]) + red[2 * LZ + a]) + red[3 * LZ + a];
        const size_t o = ((size_t)(co0 + col) * Cin + c0 + c) * taps + tap;
        v *= gscale;
        dw[o] = accumulate ? dw[o] + v : v;
      }
    }
    return;
  }
  if ((int)blk < nwblk) {
    // linear path: 256 consecutive slab entries, four z-lanes, scattered writes
    const size_t q0 = (size_t)blk * WR_BLK + (size_t)lane * 4;      // first of this thread's four entries
    const bool vec = (total & 3) == 0 && (((uintptr_t)part) & 15) == 0;
    float4 s[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (q0 < total) {
      if (vec) {
        const float* src = part + q0;
        int z = zl;
        for (; z + 12 < Z; z += 16) {
          float4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(src + (size_t)(z + 4 * u) * total);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            s[u & 1].x += v[u].x; s[u & 1].y += v[u].y; s[u & 1].z += v[u].z; s[u & 1].w += v[u].w;
          }
        }
        for (; z < Z; z += 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (size_t)z * total);
          s[0].x += v.x; s[0].y += v.y; s[0].z += v.z; s[0].w += v.w;
        }
      } else {
        for (int z = zl; z < Z; z += 4) {
          const float* src = part + (size_t)z * total + q0;
          s[0].x += src[0];
          if (q0 + 1 < total) s[0].y += src[1];
          if (q0 + 2 < total) s[0].z += src[2];
          if (q0 + 3 < total) s[0].w += src[3];
        }
      }
    }
    *reinterpret_cast<float4*>(red + zl * LZ + lane * 4) = make_float4(s[0].x + s[1].x, s[0].y + s[1].y, s[0].z + s[1].z, s[0].w + s[1].w);
    __syncthreads();
    const size_t idx = (size_t)blk * WR_BLK + threadIdx.x;
    if (idx < total) {
      const int k_ = (int)(idx / Cout);
      const int tap_ = k_ / cin_ld, ci_ = k_ - tap_ * cin_ld;
      if (ci_ < Cin && tap_ < KH * KW) {          // padded slab rows carry no gradient
        float v = ((red[0 * LZ + threadIdx.x] + red[1 * LZ + threadIdx.x]) + red[2 * LZ + threadIdx.x]) + red[3 * LZ + threadIdx.x];
        const int co = (int)(idx - (size_t)k_ * Cout);
        const size_t o = wgrad_out_index(tap_, ci_, co, Cin, Cout, KH, KW, layout);
        v *= gscale;
        dw[o] = accumulate ? dw[o] + v : v;
      }
    }
    return;
  }
  // bias entries: 256 per block, four z-lanes
  if (!(db && dbpart)) return;
  const size_t c = (size_t)(blk - nwblk) * WR_BLK + lane * 4;
  float4 sb = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int z = zl; z < Z; z += 4) {
    const float* src = dbpart + (size_t)z * Cout + c;
    if (c < (size_t)Cout) sb.x += src[0];
    if (c + 1 < (size_t)Cout) sb.y += src[1];
    if (c + 2 < (size_t)Cout) sb.z += src[2];
    if (c + 3 < (size_t)Cout) sb.w += src[3];
  }
  *reinterpret_cast<float4*>(red + zl * LZ + lane * 4) = sb;
  __syncthreads();
  const size_t o = (size_t)(blk - nwblk) * WR_BLK + threadIdx.x;
  if (o < (size_t)Cout) {
    const float v = ((red[0 * LZ + threadIdx.x] + red[1 * LZ + threadIdx.x]) + red[2 * LZ + threadIdx.x]) + red[3 * LZ + threadIdx.x];
    db[o] = accumulate ? db[o] + v : v;
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbpart,
                                                           int Z, int K, int Cin, int Cout, int KH, int KW, int layout,
                                                           float* dw, float* db, int accumulate, float gscale) {
  __shared__ __attribute__((aligned(16))) float red[4 * (WR_MAXR * WR_PITCH + 4)];
  wgrad_reduce_body(red, part, dbpart, Z, K, Cin, Cout, KH, KW, layout, dw, db, accumulate, gscale, blockIdx.x, 0);
}

// every slab reduce of a backward pass in ONE launch (device-resident descriptor table, like pack_program): the
// per-layer reduces were ~70 launches of ~9 us each on the weight-gradient stream
__global__ __launch_bounds__(256) void wgrad_reduce_program_kernel(const tpgsr_wgrad_reduce_desc* __restrict__ descs, int ndesc) {
  __shared__ __attribute__((aligned(16))) float red[4 * (WR_MAXR * WR_PITCH + 4)];
  __shared__ int s_d;
  if (threadIdx.x == 0) {
    int lo = 0, hi = ndesc - 1;  // last descriptor whose blk0 <= blockIdx.x
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (descs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_d = lo;
  }
  __syncthreads();
  const tpgsr_wgrad_reduce_desc d = descs[s_d];
  wgrad_reduce_body(red, d.part, d.dbpart, d.Z, d.K, d.Cin, d.Cout, d.KH, d.KW, d.layout, d.dw, d.db, d.accumulate, d.gscale,
                    blockIdx.x - (unsigned)d.blk0, d.cin_ld);
}

/* workgroups one reduce takes (a descriptor's share of a program's grid) */
extern "C" int tpgsr_wgrad_reduce_blocks2(int K, int Cin, int Cout, int KH, int KW, int layout, int cin_ld, int has_bias) {
  (void)cin_ld;
  return wr_weight_blocks(K, Cin, Cout, KH, KW, layout) + (has_bias ? cdiv(Cout, WR_BLK) : 0);
}

extern "C" int tpgsr_wgrad_reduce_program(const tpgsr_wgrad_reduce_desc* descs_dev, int ndesc, int total_blocks, void* stream) {
  TPGSR_CHECK_ARG(descs_dev && ndesc > 0 && total_blocks > 0, "tpgsr_wgrad_reduce_program: bad arguments");
  hipLaunchKernelGGL(wgrad_reduce_program_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, ndesc);
  TPGSR_LAUNCH_CHECK("tpgsr_wgrad_reduce_program");
}

extern "C" int tpgsr_wgrad_reduce(const float* part, const float* dbpart, int Z, int K, int Cin, int Cout, int KH, int KW,
                                  int layout, float* dw, float* db, int accumulate, float gscale, void* stream) {
  TPGSR_CHECK_ARG(part && dw && Z > 0 && K >= KH * KW * Cin, "tpgsr_wgrad_reduce: bad arguments");
  TPGSR_CHECK_ARG((((uintptr_t)part) & 15) == 0, "tpgsr_wgrad_reduce: slabs must be 16-byte aligned");
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(tpgsr_wgrad_reduce_blocks2(K, Cin, Cout, KH, KW, layout, 0, (db && dbpart) ? 1 : 0)), dim3(256), 0,
                     (hipStream_t)stream, part, dbpart, Z, K, Cin, Cout, KH, KW, layout, dw, db, accumulate, gscale);
  TPGSR_LAUNCH_CHECK("tpgsr_wgrad_reduce");
}

// ------------------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------------------
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, int Cout, int Cin, int KH, int KW, int transposed,
                                        float wscale, float* wt_f, float* wt_d) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Cout * Cin * KH * KW;
  if (idx >= total) return;
  int kw = idx % KW;
  size_t r = idx / KW;
  int kh = r % KH;
  r /= KH;
  int co, ci;
  if (!transposed) {
    ci = r % Cin;
    co = (int)(r / Cin);
  } else {  // source [Cin][Cout][KH][KW]; equivalent conv weight w_eq[co][ci][kh'][kw'] with flipped taps
    co = r % Cout;
    ci = (int)(r / Cout);
    kh = KH - 1 - kh;
    kw = KW - 1 - kw;
  }
  float v = w[idx] * wscale;
  if (wt_f) wt_f[((size_t)(kh * KW + kw) * Cin + ci) * Cout + co] = v;
  if (wt_d) wt_d[((size_t)((KH - 1 - kh) * KW + (KW - 1 - kw)) * Cout + co) * Cin + ci] = v;
}

extern "C" int tpgsr_pack_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, int transposed, float wscale,
                                      float* wt_f, float* wt_d, void* stream) {
  TPGSR_CHECK_ARG(w && (wt_f || wt_d), "tpgsr_pack_conv_weight: null pointer");
  size_t total = (size_t)Cout * Cin * KH * KW;
  hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                     KH, KW, transposed, wscale, wt_f, wt_d);
  TPGSR_LAUNCH_CHECK("tpgsr_pack_conv_weight");
}

__global__ void pack_tail_weight_kernel(const float* __restrict__ w, int Co, int C, int KS, float* wt_f, float* wt_d) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Co * C * KS * KS;
  if (idx >= total) return;
  int kw = idx % KS;
  size_t r = idx / KS;
  int kh = r % KS;
  r /= KS;
  int ci = r % C;
  int co = (int)(r / C);
  float v = w[idx];
  int NP = KS * Co;  // folded output columns
  int np = kw * Co + co;
  if (wt_f) wt_f[((size_t)kh * C + ci) * NP + np] = v;
  if (wt_d) wt_d[((size_t)(KS - 1 - kh) * NP + np) * C + ci] = v;
}

extern "C" int tpgsr_pack_tail_weight(const float* w, int Co, int C, int KS, float* wt_f, float* wt_d, void* stream) {
  TPGSR_CHECK_ARG(w && (wt_f || wt_d), "tpgsr_pack_tail_weight: null pointer");
  size_t total = (size_t)Co * C * KS * KS;
  hipLaunchKernelGGL(pack_tail_weight_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, Co, C, KS,
                     wt_f, wt_d);
  TPGSR_LAUNCH_CHECK("tpgsr_pack_tail_weight");
}

// ------------------------------------------------------------------------------------------------------
// pack program: ALL per-step operand packing of a model in one launch (a device-resident descriptor table)
// ------------------------------------------------------------------------------------------------------
// kind 0 (every convolution / linear weight: the bulk of a network) with <= 9 taps is packed in TILES of 32 output x 32 input channels x
// all taps through LDS: the source [Cout][Cin][taps] is read in runs of 32 * taps floats, the k-major forward operand written in runs of
// 32 output channels, the data-gradient operand in runs of 32 input channels.  Element by element (the other kinds: small) every write
// of the forward operand lands on a cache line of its own -- the student recogniser's 8.3 M parameters took 77 us a step that way.
#define PK_TILED_MAX_TAPS 9
// (large layers only: a 64 x 64 x 9 weight would be FOUR workgroups of 9216 elements -- the SR network's 25 small layers packed in 57 us
//  that way against 46 us element by element, 144 workgroups each)
__host__ __device__ __forceinline__ bool pack_tiled(int kind, int Cout, int Cin, int KH, int KW) {
  return kind == 0 && KH * KW <= PK_TILED_MAX_TAPS && (long long)Cout * Cin >= 65536;
}
__host__ __device__ __forceinline__ int pack_desc_blocks(int kind, int Cout, int Cin, int KH, int KW, long long numel) {
  if (pack_tiled(kind, Cout, Cin, KH, KW)) return ((Cout + 31) / 32) * ((Cin + 31) / 32);
  return (int)((numel + 255) / 256);
}
extern "C" int tpgsr_pack_blocks(int kind, int Cout, int Cin, int KH, int KW, long long numel) {
  return pack_desc_blocks(kind, Cout, Cin, KH, KW, numel);
}

__global__ __launch_bounds__(256) void pack_program_kernel(const tpgsr_pack_desc* __restrict__ descs, int ndesc) {
  __shared__ int s_d;
  __shared__ float tile[32 * (32 * PK_TILED_MAX_TAPS + 1)];
  if (threadIdx.x == 0) {
    int lo = 0, hi = ndesc - 1;  // last descriptor whose blk0 <= blockIdx.x
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (descs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_d = lo;
  }
  __syncthreads();
  const tpgsr_pack_desc d = descs[s_d];
  if (pack_tiled(d.kind, d.Cout, d.Cin, d.KH, d.KW)) {
    const int taps = d.KH * d.KW, R = 32 * taps, pitch = R | 1;
    const int nci = (d.Cin + 31) / 32;
    const int b = (int)blockIdx.x - d.blk0;
    const int co0 = (b / nci) * 32, ci0 = (b - (b / nci) * nci) * 32;
    const int cw = min(32, d.Cin - ci0) * taps;        // valid floats of a source run
    for (int e = threadIdx.x; e < 32 * R; e += 256) {
      const int row = e / R, pos = e - row * R;
      float v = 0.f;
      if (co0 + row < d.Cout && pos < cw) v = d.src[((size_t)(co0 + row) * d.Cin + ci0) * taps + pos] * d.wscale;
      tile[row * pitch + pos] = v;
    }
    __syncthreads();
    const int cin_ld = d.cin_ld > 0 ? d.cin_ld : d.Cin, d_ld = d.d_ld > 0 ? d.d_ld : d.Cin;
    if (d.dst_f) {
      for (int e = threadIdx.x; e < 32 * R; e += 256) {
        const int co_l = e & 31, rest = e >> 5;
        const int ci_l = rest & 31, tap = rest >> 5;
        if (co0 + co_l < d.Cout && ci0 + ci_l < d.Cin)
          d.dst_f[((size_t)tap * cin_ld + ci0 + ci_l) * d.f_ld + d.f_coff + co0 + co_l] = tile[co_l * pitch + ci_l * taps + tap];
      }
    }
    if (d.dst_d) {
      for (int e = threadIdx.x; e < 32 * R; e += 256) {
        const int ci_l = e & 31, rest = e >> 5;
        const int co_l = rest & 31, tap = rest >> 5;
        const int kh = tap / d.KW, kw = tap - kh * d.KW;
        if (co0 + co_l < d.Cout && ci0 + ci_l < d.Cin)
          d.dst_d[((size_t)((d.KH - 1 - kh) * d.KW + (d.KW - 1 - kw)) * d.Cout + co0 + co_l) * d_ld + ci0 + ci_l] = tile[co_l * pitch + ci_l * taps + tap];
      }
    }
    return;
  }
  long long idx = (long long)(blockIdx.x - d.blk0) * 256 + threadIdx.x;
  if (idx >= d.numel) return;
  if (d.kind == 5) {  // composed GruBlock operand: one 64-term dot product per output element
    const int U = d.KH;             // conv1 output channels = GRU input size
    const int g = (int)(idx / d.Cin), ci = (int)(idx - (long long)g * d.Cin);
    const float* wr = d.src + (size_t)g * U;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int u = 0; u < U; u += 4) {
      a0 = fmaf(wr[u], d.src2[(size_t)u * d.Cin + ci], a0);
      a1 = fmaf(wr[u + 1], d.src2[(size_t)(u + 1) * d.Cin + ci], a1);
      a2 = fmaf(wr[u + 2], d.src2[(size_t)(u + 2) * d.Cin + ci], a2);
      a3 = fmaf(wr[u + 3], d.src2[(size_t)(u + 3) * d.Cin + ci], a3);
    }
    const float v = (a0 + a1) + (a2 + a3);
    if (d.dst_f) d.dst_f[(size_t)ci * d.f_ld + d.f_coff + g] = v;
    if (d.dst_d) d.dst_d[(size_t)(d.f_coff + g) * d.Cin + ci] = v;
    return;
  }
  if (d.kind == 6) {
    const int U = d.KH, g = (int)idx;
    const float* wr = d.src + (size_t)g * U;
    float a0 = 0.f, a1 = 0.f;
    for (int u = 0; u < U; u += 2) {
      a0 = fmaf(wr[u], d.src2[u], a0);
      a1 = fmaf(wr[u + 1], d.src2[u + 1], a1);
    }
    d.dst_f[d.f_coff + g] = (a0 + a1) + d.src3[g];
    return;
  }
  float v = d.src[idx] * d.wscale;
  if (d.kind == 2) {  // plain copy
    d.dst_f[idx] = v;
    return;
  }
  int kw = idx % d.KW;
  long long r = idx / d.KW;
  int kh = r % d.KH;
  r /= d.KH;
  if (d.kind == 1) {  // folded tail conv: src [Co][C][KS][KS]
    int ci = r % d.Cin;
    int co = (int)(r / d.Cin);
    int NP = d.KH * d.Cout, np = kw * d.Cout + co;  // here Cout = Co, KH = KW = KS
    if (d.dst_f) d.dst_f[((size_t)kh * d.Cin + ci) * NP + np] = v;
    if (d.dst_d) d.dst_d[((size_t)(d.KH - 1 - kh) * NP + np) * d.Cin + ci] = v;
    return;
  }
  if (d.kind == 7) {  // folded DATA-GRADIENT operand of a KS x KS convolution with few input channels: src [Cout][Cin][KS][KS]
    // (block1, model/tsrn.py:28: 4 -> 64, 9 x 9).  dx = conv(dy, flipped taps) run as a KS x 1 convolution over dy's Cout channels with the
    // KS kw-taps folded into the columns, k = kh' Cout + c, column = kw' Cin + ci, value = w[c][ci][KS-1-kh'][KS-1-kw'];
    // tpgsr_shiftsum_nhwc adds the KS column groups back up
    int ci = r % d.Cin;
    int c = (int)(r / d.Cin);
    int NP = d.KW * d.Cin;
    d.dst_f[((size_t)(d.KH - 1 - kh) * d.Cout + c) * NP + (d.KW - 1 - kw) * d.Cin + ci] = v;
    return;
  }
  if (d.kind == 4) {  // ConvTranspose2d weight [Cin][Cout][3][3] on an H=1 strip: only the kh=1 row ever meets data
    int co = r % d.Cout;
    int ci = (int)(r / d.Cout);
    if (kh != 1) return;
    int kwp = d.KW - 1 - kw;  // tap of the equivalent stride-1 conv over the zero-dilated strip
    if (d.dst_f) d.dst_f[((size_t)kwp * (d.cin_ld > 0 ? d.cin_ld : d.Cin) + ci) * d.f_ld + d.f_coff + co] = v;
    if (d.dst_d) d.dst_d[((size_t)kw * d.Cout + co) * (d.d_ld > 0 ? d.d_ld : d.Cin) + ci] = v;   // strided-conv operand of the data gradient
    return;
  }
  int co, ci;
  if (d.kind == 0) {
    ci = r % d.Cin;
    co = (int)(r / d.Cin);
  } else {  // kind 3: ConvTranspose2d weight [Cin][Cout][KH][KW] -> equivalent conv (flipped taps)
    co = r % d.Cout;
    ci = (int)(r / d.Cout);
    kh = d.KH - 1 - kh;
    kw = d.KW - 1 - kw;
  }
  if (d.dst_f) d.dst_f[((size_t)(kh * d.KW + kw) * (d.cin_ld > 0 ? d.cin_ld : d.Cin) + ci) * d.f_ld + d.f_coff + co] = v;
  if (d.dst_d) d.dst_d[((size_t)((d.KH - 1 - kh) * d.KW + (d.KW - 1 - kw)) * d.Cout + co) * (d.d_ld > 0 ? d.d_ld : d.Cin) + ci] = v;
}

// chain rule of the composed GruBlock operand (see tpgsr_compose_bwd_desc): one thread per gradient element
__global__ __launch_bounds__(256) void compose_bwd_program_kernel(const tpgsr_compose_bwd_desc* __restrict__ descs, int ndesc) {
  __shared__ int s_d;
  if (threadIdx.x == 0) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (descs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    s_d = lo;
  }
  __syncthreads();
  const tpgsr_compose_bwd_desc d = descs[s_d];
  const int Cin = d.Cin, U = d.U, G = d.G;
  int idx = (int)(blockIdx.x - d.blk0) * 256 + threadIdx.x;
  const int n_w1 = U * Cin, n_b1 = U, n_wih = 2 * G * U, n_bih = 2 * G;
  auto wih = [&](int g, int u) { return g < G ? d.wih0[(size_t)g * U + u] : d.wih1[(size_t)(g - G) * U + u]; };
  if (idx < n_w1) {   // dW1[u][ci] += sum_g Wih[g][u] * dWc[g][ci]
    const int u = idx / Cin, ci = idx - u * Cin;
    float a0 = 0.f, a1 = 0.f;
    for (int g = 0; g < 2 * G; g += 2) {
      a0 = fmaf(wih(g, u), d.dWc[(size_t)g * Cin + ci], a0);
      a1 = fmaf(wih(g + 1, u), d.dWc[(size_t)(g + 1) * Cin + ci], a1);
    }
    d.dW1[idx] += a0 + a1;
    return;
  }
  idx -= n_w1;
  if (idx < n_b1) {
    float a0 = 0.f, a1 = 0.f;
    for (int g = 0; g < 2 * G; g += 2) {
      a0 = fmaf(wih(g, idx), d.dbc[g], a0);
      a1 = fmaf(wih(g + 1, idx), d.dbc[g + 1], a1);
    }
    d.db1[idx] += a0 + a1;
    return;
  }
  idx -= n_b1;
  if (idx < n_wih) {  // dWih[g][u] += sum_ci dWc[g][ci] * W1[u][ci]
    const int g = idx / U, u = idx - g * U;
    const float* a = d.dWc + (size_t)g * Cin;
    const float* b = d.W1 + (size_t)u * Cin;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int ci = 0; ci < Cin; ci += 4) {
      a0 = fmaf(a[ci], b[ci], a0);
      a1 = fmaf(a[ci + 1], b[ci + 1], a1);
      a2 = fmaf(a[ci + 2], b[ci + 2], a2);
      a3 = fmaf(a[ci + 3], b[ci + 3], a3);
    }
    float* dst = g < G ? d.dwih0 + (size_t)g * U + u : d.dwih1 + (size_t)(g - G) * U + u;
    *dst += ((a0 + a1) + (a2 + a3)) + d.dbc[g] * d.b1[u];   // conv output = W1 x + b1
    return;
  }
  idx -= n_wih;
  if (idx < n_bih) {
    float* dst = idx < G ? d.dbih0 + idx : d.dbih1 + (idx - G);
    *dst += d.dbc[idx];
  }
}

extern "C" int tpgsr_compose_bwd_blocks(int Cin, int U, int G) { return cdiv((long long)U * Cin + U + 2ll * G * U + 2 * G, 256); }

extern "C" int tpgsr_compose_bwd_program(const tpgsr_compose_bwd_desc* descs_dev, int ndesc, int total_blocks, void* stream) {
  TPGSR_CHECK_ARG(descs_dev && ndesc > 0 && total_blocks > 0, "tpgsr_compose_bwd_program: bad arguments");
  hipLaunchKernelGGL(compose_bwd_program_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, ndesc);
  TPGSR_LAUNCH_CHECK("tpgsr_compose_bwd_program");
}

extern "C" int tpgsr_pack_program(const tpgsr_pack_desc* descs_dev, int ndesc, int total_blocks, void* stream) {
  TPGSR_CHECK_ARG(descs_dev && ndesc > 0 && total_blocks > 0, "tpgsr_pack_program: bad arguments");
  hipLaunchKernelGGL(pack_program_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, ndesc);
  TPGSR_LAUNCH_CHECK("tpgsr_pack_program");
}

extern "C" int tpgsr_copy(const float* src, float* dst, long long n, void* stream) {
  TPGSR_CHECK_ARG(src && dst && n > 0, "tpgsr_copy: bad arguments");
  hipError_t e = hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) {
    tpgsr_set_error("tpgsr_copy: %s", hipGetErrorString(e));
    return TPGSR_ERR_LAUNCH;
  }
  return 0;
}

extern "C" int tpgsr_zero(float* dst, long long n, void* stream) {
  TPGSR_CHECK_ARG(dst && n > 0, "tpgsr_zero: bad arguments");
  hipError_t e = hipMemsetAsync(dst, 0, (size_t)n * sizeof(float), (hipStream_t)stream);
  if (e != hipSuccess) {
    tpgsr_set_error("tpgsr_zero: %s", hipGetErrorString(e));
    return TPGSR_ERR_LAUNCH;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------
// diagnostic: register-only fp32 MFMA loop (no memory traffic) -- the achievable v_mfma_f32_32x32x2_f32 rate of this
// chip at its sustained clock; bench.py reports it next to the datasheet peak
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfma_probe_kernel(float* out, int iters, float a0, float b0) {
  floatx16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
  float a = a0 + (float)(threadIdx.x & 7), b = b0 + (float)(threadIdx.x & 3);
  for (int it = 0; it < iters; ++it) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(b, a, acc1, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i];
  if (s == 12345.678f) out[0] = s;   // keep the loop alive
}

extern "C" int tpgsr_mfma_probe(float* out, int blocks, int iters, void* stream) {
  TPGSR_CHECK_ARG(out && blocks > 0 && iters > 0, "tpgsr_mfma_probe: bad arguments");
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters, 1.0f, 0.5f);
  TPGSR_LAUNCH_CHECK("tpgsr_mfma_probe");
}
