// Device code shared by the BiGRU kernels (gru.hip: the scans over precomputed input projections and back-propagation through time;
// gru_proj.hip: the forward scan with the GruBlock's input projection computed in the same launch): sequence geometry, the gate
// functions of the recurrence, packed-FMA helpers and -- at the end of the file -- the time step itself, forward and backward, for every
// kernel that runs it.  GruBlock: model/tsrn.py:491-508.
#pragma once
#include "common.h"

#define GRU_H 32      // the hidden size of the files that are built for one size only (gru_proj.hip, gru_wgrad.hip)

struct SeqGeom {
  int base;    // pixel index of t = 0 (32-bit: the launchers bound N H W 8 U, the largest index, by 2^31 -- 64-bit multiplies were ~20 instructions of a step)
  int stride;  // pixel stride between time steps
  int T;
  bool active;
};

__device__ __forceinline__ SeqGeom seq_geom(int s, int N, int H, int W, int axis) {
  SeqGeom g;
  int nseq = axis == 0 ? N * H : N * W;
  g.active = s < nseq;
  if (!g.active) s = 0;
  if (axis == 0) {
    g.base = s * W;
    g.stride = 1;
    g.T = W;
  } else {
    int n = s / W, col = s - n * W;
    g.base = n * H * W + col;
    g.stride = W;
    g.T = H;
  }
  return g;
}

// Gate functions of the recurrence.  A time step is ONE dependent instruction stream per wave (a step of the W-axis scan runs with at most
// one wave per SIMD), so its length in instructions is its latency: libm's expf + expm1f + three IEEE divisions were ~110 of the ~190
// instructions of a step.  These keep libm-level accuracy in a third of that:
//   e^x   = v_exp_f32(t) * (1 + ln2 * lo),  t = fl(x log2e), lo = the exact rounding error of t + x * (log2e - fl(log2e))   (6 instructions;
//           the bare v_exp_f32(x * log2e) loses |x| * 6e-8 relative -- common.h's note on what that did to the text-prior gradient)
//   1 / d = v_rcp_f32 + one Newton step (3 instructions, <= 1 ulp)
//   tanh  = x * P(x^2) for |x| < 0.35 (odd Taylor polynomial to x^11: 5e-9 relative), (1 - q) / (1 + q) with q = e^(-2|x|) elsewhere
// Checked against fp64 over the gates' range by tests/test_gru_gate_math_gpu.py: worst case 3.5 ulp (sigmoid) / 4.5 ulp (tanh, where
// 1 - q cancels one bit), against 2 ulp of the libm path; mean error 0.4 ulp either way.
__device__ __forceinline__ float gru_exp(float x) {
  const float t = x * 1.44269504088896341f;
  float lo = __builtin_fmaf(x, 1.44269504088896341f, -t);
  lo = __builtin_fmaf(x, 1.925963033500011e-08f, lo);
  const float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, lo * 0.6931471805599453f, e);
}
__device__ __forceinline__ float gru_rcp(float d) {      // d finite, |d| in [2^-126, 2^126]
  const float r = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(__builtin_fmaf(-d, r, 1.f), r, r);
}
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 mk2(float x, float y) {
  f2 v;
  v.x = x;
  v.y = y;
  return v;
}

// (v, v) for a packed multiply-add when v is an ODD component (.y / .w) of a float4 an LDS read has just returned.  mk2(v, v) compiles to
// v_pk_fma_f32 ... op_sel:[0,1,0] on the returned register pair -- the LOW half of the instruction takes the pair's ODD register -- and
// that form read the register as ZERO in lanes 48-63 (while the high half of the same instruction read it correctly) once in ~10^4
// time steps when three scanning waves shared a SIMD: measured term by term in round 6 (profiles/r06_gru_proj_root_cause.md; every other
// operand form of the scans -- even components with op_sel_hi, natural (x, y) pairs, a component copied by v_mov -- never failed in
// 10^6 sequence launches).  The copy costs one v_mov_b32 per use; results are the same bits.
__device__ __forceinline__ f2 gru_dup_odd(float v) {
  float c;
  asm("v_mov_b32 %0, %1" : "=v"(c) : "v"(v));
  return mk2(c, c);
}

// TWO sigmoids in lock step (the r and z gates of a time step), component for component the operations of gru_rcp(1 + gru_exp(min(-x, 80)))
// as packed instructions (v_pk_mul / v_pk_fma / v_pk_add; v_exp and v_rcp back to back).  A lone wave pays ~10 cycles per DEPENDENT VALU
// instruction and 3-5 per independent one (tools/lab/valu_rate.hip): the two sigmoids one after the other -- the compiler even scheduled the
// second one behind the tanh that needs only the first -- were ~250 cycles of a ~1350-cycle step; in lock step they are one chain.
__device__ __forceinline__ f2 gru_sigmoid2(f2 x) {
  const f2 nx = mk2(fminf(-x.x, 80.f), fminf(-x.y, 80.f));
  const f2 l2e = mk2(1.44269504088896341f, 1.44269504088896341f);
  const f2 t = nx * l2e;
  f2 lo = pk_fma(nx, l2e, -t);
  lo = pk_fma(nx, mk2(1.925963033500011e-08f, 1.925963033500011e-08f), lo);
  const f2 e = mk2(__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y));
  const f2 d = mk2(1.f, 1.f) + pk_fma(e, lo * mk2(0.6931471805599453f, 0.6931471805599453f), e);
  const f2 r = mk2(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y));
  return pk_fma(pk_fma(-d, r, mk2(1.f, 1.f)), r, r);
}
__device__ __forceinline__ float gru_sigmoid(float x) { return gru_sigmoid2(mk2(x, x)).x; }
// one sigmoid, the same operations as a component of gru_sigmoid2 (the LSTM cells of lstm_seq.hip / crnn.hip: four gates per unit)
__device__ __forceinline__ float gru_sigmoid1(float x) { return gru_rcp(1.f + gru_exp(fminf(-x, 80.f))); }
// BRANCH-FREE: both forms are computed and one is selected.  Left to itself the compiler sinks them into the two sides of a divergent
// branch (s_cbranch_execz): a scheduling barrier in the middle of the step, with both sides executed by every wave anyway (the lanes of a
// wave are 64 different hidden units).  The empty asm pins both values in front of the select.
__device__ __forceinline__ float gru_tanh(float x) {
  const float q = gru_exp(-2.f * fabsf(x));
  float big = (1.f - q) * gru_rcp(1.f + q);
  const float x2 = x * x;
  float p = __builtin_fmaf(x2, -1382.f / 155925.f, 62.f / 2835.f);
  p = __builtin_fmaf(x2, p, -17.f / 315.f);
  p = __builtin_fmaf(x2, p, 2.f / 15.f);
  p = __builtin_fmaf(x2, p, -1.f / 3.f);
  p = __builtin_fmaf(x2, p, 1.f);
  float small = x * p;
  asm volatile("" : "+v"(small), "+v"(big));
  return fabsf(x) < 0.35f ? small : copysignf(big, x);
}

// ------------------------------------------------------------------------------------------------------
// The recurrence, once.  U = hidden size (32 | 64).
// ------------------------------------------------------------------------------------------------------
// Lane maps.  A scanning wave exchanges per-unit values through wave-private, parity-double-buffered LDS slots: State = one float per
// unit (the hidden state; dghn), Pairs = two (dr, dz).  put() = where this lane writes its own, get() = where its direction's vector starts.
//   U = 32: one wavefront per sequence, lanes 0-31 the forward direction, 32-63 the reverse one; State [parity][dir * 32 + unit]
//           (put() indexes with the lane id itself: the compiler does not see that d * 32 + j is the same number).
//   U = 64: one wavefront per (sequence, direction), two per workgroup (wave 0 forward, wave 1 reverse), independent recurrences: nothing
//           ever waits for the other wave, no workgroup barrier anywhere; State [dir][parity][unit].
// The slots are declared with these array types, not as flat floats: the index form decides the address arithmetic of every step.
// Either way a slot belongs to ONE wave, whose LDS operations execute in order: the per-step barrier is a compiler barrier only.
template <int U>
struct GruLanes;
template <>
struct GruLanes<32> {
  static constexpr int THREADS = 64;
  typedef float State[2][64];         // [parity][dir * 32 + unit]
  typedef float Pairs[2][2][64];      // [parity][dir][unit][2]
  int lane, d, j;      // d = direction, j = hidden unit
  __device__ __forceinline__ GruLanes(unsigned tid) : lane(tid & 63), d(lane >> 5), j(lane & 31) {}
  __device__ __forceinline__ float* put(State& s, int parity) const { return &s[parity][lane]; }
  __device__ __forceinline__ const float4* get(const State& s, int parity) const { return reinterpret_cast<const float4*>(&s[parity][d * 32]); }
  __device__ __forceinline__ float2* put(Pairs& s, int parity) const { return reinterpret_cast<float2*>(&s[parity][d][2 * j]); }
  __device__ __forceinline__ const float4* get(const Pairs& s, int parity) const { return reinterpret_cast<const float4*>(&s[parity][d][0]); }
};
template <>
struct GruLanes<64> {
  static constexpr int THREADS = 128;
  typedef float State[2][2][64];      // [dir][parity][unit]
  typedef float Pairs[2][2][128];     // [dir][parity][unit][2]
  int d, j;
  __device__ __forceinline__ GruLanes(unsigned tid) : d(__builtin_amdgcn_readfirstlane(tid >> 6)), j(tid & 63) {}      // (d: wave-uniform)
  __device__ __forceinline__ float* put(State& s, int parity) const { return &s[d][parity][j]; }
  __device__ __forceinline__ const float4* get(const State& s, int parity) const { return reinterpret_cast<const float4*>(&s[d][parity][0]); }
  __device__ __forceinline__ float2* put(Pairs& s, int parity) const { return reinterpret_cast<float2*>(&s[d][parity][2 * j]); }
  __device__ __forceinline__ const float4* get(const Pairs& s, int parity) const { return reinterpret_cast<const float4*>(&s[d][parity][0]); }
};

// The step's pieces are LOOP-FREE functions of scalars and register arrays; the k loops around gru_mac / gru_mac_t and the W_hh loads
// stay in the kernels.  A function that holds an unrolled loop, or takes an f2 / float4 by value into the gate math, is simplified
// by the compiler on its own before it is inlined and the step comes out scheduled differently (and with other register counts) than
// the same lines written in the kernel; in this form every scan instantiation is the code of the hand-kept copies it replaced.

// one k-step (state components 4k .. 4k+3) of W_hh h for one unit: six independent packed-FMA chains.  wrz = row j of W_hr / W_hz
// interleaved (one packed FMA feeds both gates), wn2 = row j of W_hn as k-pairs; hv = the direction's state vector, a broadcast
// ds_read_b128.  The odd components go through gru_dup_odd, NOT mk2(hv.y, hv.y) (see there).
// Afterwards: (W_hr h, W_hz h) = (a0 + a1) + (a2 + a3), W_hn h = (n0 + n1).x + (n0 + n1).y.
template <int U>
__device__ __forceinline__ void gru_mac(const f2 (&wrz)[U], const f2 (&wn2)[U / 2], int k, const float4 hv, f2& a0, f2& a1, f2& a2, f2& a3,
                                        f2& n0, f2& n1) {
  a0 = pk_fma(wrz[4 * k], mk2(hv.x, hv.x), a0);
  a1 = pk_fma(wrz[4 * k + 1], gru_dup_odd(hv.y), a1);
  a2 = pk_fma(wrz[4 * k + 2], mk2(hv.z, hv.z), a2);
  a3 = pk_fma(wrz[4 * k + 3], gru_dup_odd(hv.w), a3);
  n0 = pk_fma(wn2[2 * k], mk2(hv.x, hv.y), n0);
  n1 = pk_fma(wn2[2 * k + 1], mk2(hv.z, hv.w), n1);
}
// Gate math == nn.GRU:  r = s(gi_r + W_hr h + b_hr), z likewise, n = tanh(gi_n + r * an), an = W_hn h + b_hn, h' = (1 - z) * n + z * h.
// wr / wz / wn = the three hidden-side products.  What back-propagation needs of a step is what this returns.
struct GruGates {
  float r, z, n, an;
};
__device__ __forceinline__ GruGates gru_gate_update(float gi_r, float gi_z, float gi_n, float wr, float wz, float wn, float br, float bz,
                                                    float bn, float& h) {
  GruGates q;
  q.an = bn + wn;
  const f2 sg = gru_sigmoid2(mk2(gi_r + (br + wr), gi_z + (bz + wz)));      // both gates in lock step
  q.r = sg.x;
  q.z = sg.y;
  q.n = gru_tanh(__builtin_fmaf(q.r, q.an, gi_n));
  h = __builtin_fmaf(q.z, h, (1.f - q.z) * q.n);      // (explicit contraction)
  return q;
}

// back-propagation through one step: the gradients of the three gates' pre-activations from dh = d(loss) / d(h of this step), and the
// hidden side of the n gate, dghn = dn_pre * r
struct GruGateGrads {
  float dr_pre, dz_pre, dn_pre, dghn;
};
__device__ __forceinline__ GruGateGrads gru_gate_grads(float dh, float hprev, float r, float z, float n, float an) {
  GruGateGrads q;
  q.dn_pre = dh * (1.f - z) * (1.f - n * n);
  q.dz_pre = dh * (hprev - n) * z * (1.f - z);
  q.dr_pre = q.dn_pre * an * r * (1.f - r);
  q.dghn = q.dn_pre * r;
  return q;
}
// one k-step (units 4k .. 4k+3) of W_hh^T (dr_pre, dz_pre, dghn) for one unit.  trz = column j of W_hr / W_hz interleaved, tn2 = column j
// of W_hn as row pairs; a, b = the direction's (dr, dz) pairs of the four units, e = their dghn.
// Afterwards: sum = ((c0 + c1) + (c2 + c3)) + (e0 + e1), dh_prev[j] = sum.x + sum.y.
template <int U>
__device__ __forceinline__ void gru_mac_t(const f2 (&trz)[U], const f2 (&tn2)[U / 2], int k, const float4 a, const float4 b, const float4 e,
                                          f2& c0, f2& c1, f2& c2, f2& c3, f2& e0, f2& e1) {
  c0 = pk_fma(trz[4 * k], mk2(a.x, a.y), c0);
  c1 = pk_fma(trz[4 * k + 1], mk2(a.z, a.w), c1);
  c2 = pk_fma(trz[4 * k + 2], mk2(b.x, b.y), c2);
  c3 = pk_fma(trz[4 * k + 3], mk2(b.z, b.w), c3);
  e0 = pk_fma(tn2[2 * k], mk2(e.x, e.y), e0);
  e1 = pk_fma(tn2[2 * k + 1], mk2(e.z, e.w), e1);
}
