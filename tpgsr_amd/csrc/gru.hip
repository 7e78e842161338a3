// Fused bidirectional GRU time-step kernels for the recurrent residual blocks (GruBlock, model/tsrn.py:491-508), hidden size U = 32
// (the default network) or 64 (TSRN / TSRN_TL with hidden_units = 64: a 128-channel trunk): ONE forward scan and ONE back-propagation
// through time, templated on U; the step itself is gru_common.h's, shared with gru_proj.hip.
// A lane owns one hidden unit of one direction and keeps its three W_hh rows (3 U floats; the backward scan: columns) in VGPRs for
// all T steps.  Two lane maps (GruLanes<U>, gru_common.h):
//   U = 32  one wavefront per sequence, one wave per workgroup: lanes 0-31 run the forward direction, lanes 32-63 the reverse one;
//   U = 64  one wavefront per (sequence, DIRECTION), two waves per workgroup (wave 0 forward, wave 1 reverse).  The two waves are
//           independent recurrences: nothing ever waits for the other (no workgroup barrier anywhere).
// The hidden state is exchanged through a wave-private, double-buffered LDS slot (broadcast ds_read_b128), the output is written
// straight into the NHWC map, so the reference's permute/contiguous/view copies and its `.transpose(-1,-2)` (axis = 1) never exist.
// The forward pass also stores the gate values (r, z, n, W_hn h + b_hn) of every step, so back-propagation through time has nothing
// to recompute: per step it is one LDS exchange of the gate gradients and the 3 U-term W_hh^T product.  The dot products run as
// v_pk_fma_f32 (two fp32 FMAs per lane per issue).  gi = W_i x + b_i is precomputed by the MFMA GEMM (tpgsr_conv_fwd).
// Buffers: gi / dgi / dgh [P][6 U], column = dir * 3 U + gate * U + j; h [P][2 U], column = dir * U + j; gates [P][8 U], column =
// dir * 4 U + q * U + j.
#include "gru_common.h"
#include <stdlib.h>
#include <type_traits>

extern "C" __global__ void gru_gate_math_probe_kernel(const float* x, float* sg, float* th, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    sg[i] = gru_sigmoid(x[i]);
    th[i] = gru_tanh(x[i]);
  }
}
/* test hook (tests/test_gru_gate_math_gpu.py): the recurrence's sigmoid / tanh over n values */
extern "C" int tpgsr_gru_gate_math_probe(const float* x, float* sg, float* th, int n, void* stream) {
  TPGSR_CHECK_ARG(x && sg && th && n > 0, "tpgsr_gru_gate_math_probe: bad arguments");
  hipLaunchKernelGGL(gru_gate_math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, sg, th, n);
  TPGSR_LAUNCH_CHECK("tpgsr_gru_gate_math_probe");
}

// LAB BUILDS ONLY (-DTPGSR_LAB, tools/lab/gru_bwd_probe.py): parts of bigru_bwd_kernel switched off to time the rest -- bit 0 = operands not
// loaded (constants), 1 = nothing stored, 2 = no LDS exchange / W_hh^T product (dh_carry = dh z), 3 = no time steps at all (launch + W_hh
// load).  Results are garbage with any bit set.
#ifdef TPGSR_LAB
__device__ int g_gru_dbg = 0;
extern "C" int tpgsr_gru_debug(int bits) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gru_dbg), &bits, sizeof(bits)) == hipSuccess ? 0 : TPGSR_ERR_LAUNCH;
}
#define GRU_DBG() __builtin_amdgcn_readfirstlane(g_gru_dbg)
#else
#define GRU_DBG() 0
#endif

// EXACT: T is a multiple of PF (both scan lengths of the 16 x 64 map with the default PF = 8): no per-step bounds tests, the ring's
// refill is switched off per group of PF steps.  Offsets are running 32-bit element indices advanced by a constant per step.
template <int U, int PF, bool EXACT>
__global__ __launch_bounds__(GruLanes<U>::THREADS) void bigru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                                          const float* __restrict__ b_hh, int N, int H, int W, int axis,
                                                                          float* __restrict__ h_out, float* __restrict__ gates) {
  __shared__ __attribute__((aligned(16))) typename GruLanes<U>::State hs;      // the state, double-buffered by step parity
  const GruLanes<U> L(threadIdx.x);
  const int d = L.d, j = L.j;
  const SeqGeom g = seq_geom(blockIdx.x, N, H, W, axis);
  if (!g.active) return;        // (all waves of the workgroup alike, and nobody waits for anybody)
  // row j of W_hr / W_hz interleaved (one packed FMA feeds both gates), row j of W_hn as k-pairs
  f2 wrz[U], wn2[U / 2];
  {
    const float* pr = w_hh + ((size_t)(d * 3 * U + 0 * U + j)) * U;
    const float* pz = w_hh + ((size_t)(d * 3 * U + 1 * U + j)) * U;
    const float* pn = w_hh + ((size_t)(d * 3 * U + 2 * U + j)) * U;
#pragma unroll
    for (int k = 0; k < U; ++k) wrz[k] = mk2(pr[k], pz[k]);
#pragma unroll
    for (int k = 0; k < U / 2; ++k) wn2[k] = mk2(pn[2 * k], pn[2 * k + 1]);
  }
  const float br = b_hh[d * 3 * U + j], bz = b_hh[d * 3 * U + U + j], bn = b_hh[d * 3 * U + 2 * U + j];
  float h = 0.f;
  *L.put(hs, 0) = 0.f;
  __builtin_amdgcn_wave_barrier();      // LDS operations of one wave execute in order; this only pins the compiler's order
  const int T = g.T;
  const int dpix = d == 0 ? g.stride : -g.stride;                 // pixel step in the direction's own scan order
  int pix = g.base + (d == 0 ? 0 : (T - 1) * g.stride);           // pixel of the current step
  int fpix = pix;                                                 // pixel of the next step to fetch
  // The input projections do not depend on the recurrence: they are fetched PF steps ahead through a small register ring.  One
  // step of look-ahead left the wave waiting on memory in EVERY step whenever a load took longer than a step -- i.e. always, next to
  // the other kernels of the training step (the backward kernel below learnt this first).
  struct StepIn {
    float r, z, n;
  };
  auto fetch = [&]() __attribute__((always_inline)) {
    StepIn s;
    const float* p = gi + fpix * (6 * U) + d * 3 * U + j;
    s.r = p[0]; s.z = p[U]; s.n = p[2 * U];
    fpix += dpix;
    return s;
  };
  StepIn ring[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) ring[i] = (EXACT || i < T) ? fetch() : StepIn{0.f, 0.f, 0.f};
  for (int base = 0; base < T; base += PF) {
    const bool more = base + PF < T;               // (EXACT) the next group exists: refill the ring
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int step = base + i;
      if (!EXACT && step >= T) break;             // wave-uniform
      const StepIn c = ring[i];
      if (EXACT ? more : step + PF < T) ring[i] = fetch();
      f2 a0 = mk2(0.f, 0.f), a1 = a0, a2 = a0, a3 = a0, n0 = a0, n1 = a0;
      const float4* hp = L.get(hs, i & 1);      // (PF is even: step parity = i parity)
#pragma unroll
      for (int k = 0; k < U / 4; ++k) gru_mac<U>(wrz, wn2, k, hp[k], a0, a1, a2, a3, n0, n1);
      const f2 rz = (a0 + a1) + (a2 + a3), nn = n0 + n1;
      const GruGates q = gru_gate_update(c.r, c.z, c.n, rz.x, rz.y, nn.x + nn.y, br, bz, bn, h);
      *L.put(hs, (i + 1) & 1) = h;
      h_out[pix * (2 * U) + d * U + j] = h;
      if (gates) {
        float* o = gates + pix * (8 * U) + d * 4 * U + j;
        o[0] = q.r; o[U] = q.z; o[2 * U] = q.n; o[3 * U] = q.an;
      }
      pix += dpix;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// backward through time
//   inputs : gates (r, z, n, an saved by the forward pass), h_out (saved states), dh_out (+ optional dh_out2, summed)
//   outputs: dgi [P][6 U]  = (dr_pre, dz_pre, dn_pre)   -> dW_ih, db_ih, d(input) by GEMM
//            dgh [P][6 U]  = (dr_pre, dz_pre, dn_pre*r) -> dW_hh, db_hh by GEMM against the shifted states
// ------------------------------------------------------------------------------------------------------
// COMPACT: `dgh` is [P][2 U] and receives only what differs from dgi -- the n gate's hidden-side gradient dn_pre * r of both directions
// (the r and z planes of dgh ARE dgi's: the fused GruBlock weight-gradient kernel, gru_wgrad.hip, reads them there)
template <int U, int PF, bool COMPACT, bool EXACT>
__global__ __launch_bounds__(GruLanes<U>::THREADS) void bigru_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ h_out,
                                                                          const float* __restrict__ dh_out, const float* __restrict__ dh_out2,
                                                                          const float* __restrict__ w_hh, int N, int H, int W, int axis,
                                                                          float* __restrict__ dgi, float* __restrict__ dgh) {
  static_assert(!COMPACT || U == GRU_H, "the compact hidden-side gradient feeds gru_wgrad.hip, a 32-unit kernel");
  __shared__ __attribute__((aligned(16))) typename GruLanes<U>::Pairs g_rz;   // (dr_i, dz_i) pairs
  __shared__ __attribute__((aligned(16))) typename GruLanes<U>::State g_n;        // dn_pre_i * r_i
  const GruLanes<U> L(threadIdx.x);
  const int d = L.d, j = L.j;
  const SeqGeom g = seq_geom(blockIdx.x, N, H, W, axis);
  if (!g.active) return;
  // column j of W_hr / W_hz interleaved, column j of W_hn as row pairs: dh_prev[j] = sum_i W[i][j] * dgate[i]
  f2 trz[U], tn2[U / 2];
#pragma unroll
  for (int i = 0; i < U; ++i)
    trz[i] = mk2(w_hh[((size_t)(d * 3 * U + 0 * U + i)) * U + j], w_hh[((size_t)(d * 3 * U + 1 * U + i)) * U + j]);
#pragma unroll
  for (int i = 0; i < U / 2; ++i)
    tn2[i] = mk2(w_hh[((size_t)(d * 3 * U + 2 * U + 2 * i)) * U + j], w_hh[((size_t)(d * 3 * U + 2 * U + 2 * i + 1)) * U + j]);
  const int dbg = GRU_DBG();      // (0 in a release build)
  const int T = g.T;
  if (dbg & 8) {      // (the loads above must stay alive)
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < U; ++i) acc += trz[i].x + trz[i].y + (i < U / 2 ? tn2[i].x + tn2[i].y : 0.f);
    if (acc == 12345.678f) dgi[0] = acc;
    return;
  }
  float dh_carry = 0.f;
  // steps run from the direction's LAST step to its first; dpix = pixel step in that order (the previous state sits one step further)
  const int dpix = d == 0 ? -g.stride : g.stride;
  int pix = g.base + (d == 0 ? (T - 1) * g.stride : 0);
  int fpix = pix, fstep = T - 1;
  // operands of one step: they do not depend on the recurrence, so they are fetched PF steps ahead through a small register ring (next
  // to the weight-gradient GEMMs of the side stream a load takes several times its idle latency)
  struct StepIn {
    float hprev, r, z, n, an, dho, dho2;
  };
  auto fetch = [&]() __attribute__((always_inline)) {
    StepIn s;
    s.hprev = 0.f;
    s.dho2 = 0.f;
    if (dbg & 1) {
      s.r = 0.4f; s.z = 0.6f; s.n = 0.1f; s.an = 0.2f; s.dho = 0.3f;
      fpix += dpix;
      --fstep;
      return s;
    }
    if (fstep > 0) s.hprev = h_out[(fpix + dpix) * (2 * U) + d * U + j];
    const float* p = gates + fpix * (8 * U) + d * 4 * U + j;
    s.r = p[0]; s.z = p[U]; s.n = p[2 * U]; s.an = p[3 * U];
    s.dho = dh_out[fpix * (2 * U) + d * U + j];
    // (added at the step that consumes it: `s.dho += ...` here made every step wait for ALL its outstanding loads and stores --
    //  one full memory round trip per time step in every launch with a second gradient, the look-ahead ring notwithstanding)
    if (dh_out2) s.dho2 = dh_out2[fpix * (2 * U) + d * U + j];
    fpix += dpix;
    --fstep;
    return s;
  };
  StepIn ring[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) ring[i] = (EXACT || i < T) ? fetch() : StepIn{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int base = T - 1; base >= 0; base -= PF) {
    const bool more = base - PF >= 0;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int step = base - i;                 // `step` = position in the direction's own forward order
      if (!EXACT && step < 0) break;             // wave-uniform
      const StepIn c = ring[i];
      if (EXACT ? more : step - PF >= 0) ring[i] = fetch();
      const float dh = dh_carry + (c.dho + c.dho2);
      const GruGateGrads q = gru_gate_grads(dh, c.hprev, c.r, c.z, c.n, c.an);
      const int par = i & 1;                     // (PF is even; only the alternation matters)
      *L.put(g_rz, par) = make_float2(q.dr_pre, q.dz_pre);
      *L.put(g_n, par) = q.dghn;
      if (!(dbg & 2)) {
        float* o = dgi + pix * (6 * U) + d * 3 * U + j;
        o[0] = q.dr_pre; o[U] = q.dz_pre; o[2 * U] = q.dn_pre;
        if (COMPACT) {
          dgh[pix * (2 * U) + d * U + j] = q.dghn;
        } else {
          float* o2 = dgh + pix * (6 * U) + d * 3 * U + j;
          o2[0] = q.dr_pre; o2[U] = q.dz_pre; o2[2 * U] = q.dghn;
        }
      }
      pix += dpix;
      if (dbg & 4) {
        dh_carry = dh * c.z + q.dghn;
        continue;
      }
      __builtin_amdgcn_wave_barrier();   // one wave per slot: its LDS operations execute in order; the parity double buffer is kept anyway
      const float4* prz = L.get(g_rz, par);
      const float4* pn = L.get(g_n, par);
      f2 c0 = mk2(0.f, 0.f), c1 = c0, c2 = c0, c3 = c0, e0 = c0, e1 = c0;
#pragma unroll
      for (int k = 0; k < U / 4; ++k) gru_mac_t<U>(trz, tn2, k, prz[2 * k], prz[2 * k + 1], pn[k], c0, c1, c2, c3, e0, e1);
      const f2 sum = ((c0 + c1) + (c2 + c3)) + (e0 + e1);
      dh_carry = dh * c.z + (sum.x + sum.y);
    }
  }
}

// look-ahead (in time steps) of the operand prefetch rings of both kernels: TPGSR_GRU_PF = 4 | 8 (default) | 12.  Loads and stores
// retire in order on one counter per wave, so a ring slot is only as far ahead as the stores issued before it allow.
static int g_gru_pf = [] { const char* e = getenv("TPGSR_GRU_PF"); const int v = e ? atoi(e) : 8; return (v == 4 || v == 12) ? v : 8; }();
extern "C" void tpgsr_gru_set_prefetch(int steps) { g_gru_pf = (steps == 4 || steps == 12) ? steps : 8; }

// f(PF as a std::integral_constant) for the look-ahead in force.  The 64-unit scans know 4 or 8: a ring of 12 steps does not fit next to
// 192 weight registers (the backward scan's ring holds seven values per step: the compiler spilt 25 registers to scratch), so a setting
// of 12 runs them with 8.
template <int U, typename F>
static void gru_with_lookahead(F&& f) {
  if (g_gru_pf == 4) {
    f(std::integral_constant<int, 4>());
  } else if (U == GRU_H && g_gru_pf == 12) {
    if constexpr (U == GRU_H) f(std::integral_constant<int, 12>());      // (never instantiated for 64 units)
  } else {
    f(std::integral_constant<int, 8>());
  }
}

template <int U>
static int bigru_fwd_launch(const float* gi, const float* w_hh, const float* b_hh, int N, int H, int W, int axis, float* h_out,
                            float* gates, void* stream, const char* who) {
  TPGSR_CHECK_ARG(gi && w_hh && b_hh && h_out, "%s: null pointer", who);
  TPGSR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (axis == 0 || axis == 1), "%s: bad geometry", who);
  TPGSR_CHECK_ARG((long long)N * H * W * 8 * U < (1ll << 31), "%s: map too large for the kernel's 32-bit indices", who);      // (the largest index: a gates column, P * 8 U)
  const int nseq = axis == 0 ? N * H : N * W, T = axis == 0 ? W : H;
  gru_with_lookahead<U>([&](auto pf) {
    constexpr int PF = decltype(pf)::value;
    hipLaunchKernelGGL((T % PF == 0 ? bigru_fwd_kernel<U, PF, true> : bigru_fwd_kernel<U, PF, false>), dim3(nseq),
                       dim3(GruLanes<U>::THREADS), 0, (hipStream_t)stream, gi, w_hh, b_hh, N, H, W, axis, h_out, gates);
  });
  TPGSR_LAUNCH_CHECK(who);
}

template <int U, bool COMPACT>
static int bigru_bwd_launch(const float* gates, const float* h_out, const float* dh_out, const float* dh_out2, const float* w_hh, int N,
                            int H, int W, int axis, float* dgi, float* dgh, void* stream, const char* who) {
  TPGSR_CHECK_ARG(gates && h_out && dh_out && w_hh && dgi && dgh, "%s: null pointer", who);
  TPGSR_CHECK_ARG(N > 0 && H > 0 && W > 0 && (axis == 0 || axis == 1), "%s: bad geometry", who);
  TPGSR_CHECK_ARG((long long)N * H * W * 8 * U < (1ll << 31), "%s: map too large for the kernel's 32-bit indices", who);      // (the largest index: a gates column, P * 8 U)
  const int nseq = axis == 0 ? N * H : N * W, T = axis == 0 ? W : H;
  gru_with_lookahead<U>([&](auto pf) {
    constexpr int PF = decltype(pf)::value;
    hipLaunchKernelGGL((T % PF == 0 ? bigru_bwd_kernel<U, PF, COMPACT, true> : bigru_bwd_kernel<U, PF, COMPACT, false>), dim3(nseq),
                       dim3(GruLanes<U>::THREADS), 0, (hipStream_t)stream, gates, h_out, dh_out, dh_out2, w_hh, N, H, W, axis, dgi, dgh);
  });
  TPGSR_LAUNCH_CHECK(who);
}

extern "C" int tpgsr_bigru_fwd(const float* gi, const float* w_hh, const float* b_hh, int N, int H, int W, int axis,
                               float* h_out, float* gates, void* stream) {
  return bigru_fwd_launch<32>(gi, w_hh, b_hh, N, H, W, axis, h_out, gates, stream, "tpgsr_bigru_fwd");
}

extern "C" int tpgsr_bigru_bwd(const float* gates, const float* h_out, const float* dh_out, const float* dh_out2,
                                const float* w_hh, int N, int H, int W, int axis, float* dgi, float* dgh, void* stream) {
  return bigru_bwd_launch<32, false>(gates, h_out, dh_out, dh_out2, w_hh, N, H, W, axis, dgi, dgh, stream, "tpgsr_bigru_bwd");
}

/* as tpgsr_bigru_bwd, but the hidden-side gradient is written compactly: dghn [P][64] = dn_pre * r of both directions (its r / z
 * planes equal dgi's) -- 2/3 fewer bytes written here and read by the weight gradients (tpgsr_gru_wgrad) */
extern "C" int tpgsr_bigru_bwd2(const float* gates, const float* h_out, const float* dh_out, const float* dh_out2,
                                 const float* w_hh, int N, int H, int W, int axis, float* dgi, float* dghn, void* stream) {
  return bigru_bwd_launch<32, true>(gates, h_out, dh_out, dh_out2, w_hh, N, H, W, axis, dgi, dghn, stream, "tpgsr_bigru_bwd2");
}

static int gru_hidden_ok(int hidden, const char* who) {
  TPGSR_CHECK_ARG(hidden == 32 || hidden == 64, "%s: hidden size %d (the BiGRU scans are built for 32 and 64)", who, hidden);
  return 0;
}

/* tpgsr_bigru_fwd with the hidden size as an argument: 32 (that entry point itself) or 64 */
extern "C" int tpgsr_bigru_fwd_u(const float* gi, const float* w_hh, const float* b_hh, int N, int H, int W, int axis, int hidden,
                                 float* h_out, float* gates, void* stream) {
  if (int rc = gru_hidden_ok(hidden, "tpgsr_bigru_fwd_u")) return rc;
  if (hidden == 32) return tpgsr_bigru_fwd(gi, w_hh, b_hh, N, H, W, axis, h_out, gates, stream);
  return bigru_fwd_launch<64>(gi, w_hh, b_hh, N, H, W, axis, h_out, gates, stream, "tpgsr_bigru_fwd_u");
}

/* tpgsr_bigru_bwd with the hidden size as an argument: 32 (that entry point itself) or 64; dgi / dgh [P][6 hidden] */
extern "C" int tpgsr_bigru_bwd_u(const float* gates, const float* h_out, const float* dh_out, const float* dh_out2, const float* w_hh,
                                 int N, int H, int W, int axis, int hidden, float* dgi, float* dgh, void* stream) {
  if (int rc = gru_hidden_ok(hidden, "tpgsr_bigru_bwd_u")) return rc;
  if (hidden == 32) return tpgsr_bigru_bwd(gates, h_out, dh_out, dh_out2, w_hh, N, H, W, axis, dgi, dgh, stream);
  return bigru_bwd_launch<64, false>(gates, h_out, dh_out, dh_out2, w_hh, N, H, W, axis, dgi, dgh, stream, "tpgsr_bigru_bwd_u");
}
