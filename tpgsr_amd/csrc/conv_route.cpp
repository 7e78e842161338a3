// The host-side decision of every convolution launch (conv_route.h).  No device code, no HIP call.
#include "conv_route.h"
#include <stdint.h>
#include <stdlib.h>
#include <initializer_list>

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- knobs: read once from the environment when the library is loaded ----
static bool env_off(const char* name) { const char* e = getenv(name); return e && e[0] == '0'; }
static bool env_on(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
static long long env_ll(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }

static ConvKnobs knobs_from_env() {
  ConvKnobs k;
  k.wstat = !env_off("TPGSR_CONV_WSTAT");
  const long long target = env_ll("TPGSR_WGRAD_TARGET", 0);
  k.wgrad_target = target > 0 ? target : 1024;
  k.halo3 = !env_off("TPGSR_XBF_HALO3");
  k.halo3_min_supertiles = env_ll("TPGSR_XBF_HALO3_MIN", 192);
  k.halo = !env_off("TPGSR_XBF_HALO");
  k.halo_min_taps = env_on("TPGSR_XBF_HALO_MINTAPS") ? 1 : 2;
  k.colmajor_min_bytes = 3ll << 20;
  k.panel = !env_off("TPGSR_XBF_PANEL");
  k.panel_min_m = env_ll("TPGSR_XBF_PANEL_MIN_M", 32768);
  k.panel_k192 = env_on("TPGSR_XBF_PANEL_K192");
  k.splitk = !env_off("TPGSR_XBF_SPLITK");
  k.splitk_target = (int)env_ll("TPGSR_XBF_SPLITK_TARGET", 640);
  k.splitk_min_chunks = (int)env_ll("TPGSR_XBF_SPLITK_MIN_CHUNKS", 6);
  k.splitk_max_tiles = (int)env_ll("TPGSR_XBF_SPLITK_MAX_TILES", 256);
  k.splitk_min_k = (int)env_ll("TPGSR_XBF_SPLITK_MIN_K", 24);
  k.splitk_over_halo = !env_off("TPGSR_XBF_SPLITK_OVER_HALO");
  k.wgrad3 = !env_off("TPGSR_XBF_WGRAD3");
  k.wgrad_halo = !env_off("TPGSR_XBF_WGRAD_HALO");
  k.wgrad_halo_minwork = env_ll("TPGSR_XBF_WGRAD_HALO_MINWORK", 16384);
  return k;
}
ConvKnobs g_conv_knobs = knobs_from_env();

extern "C" void tpgsr_halo3_set_enabled(int on) { g_conv_knobs.halo3 = on ? 1 : 0; }
extern "C" void tpgsr_halo_set_min_taps(int v) { g_conv_knobs.halo_min_taps = v < 1 ? 1 : v; }
extern "C" void tpgsr_halo_set_colmajor_min_bytes(long long v) { g_conv_knobs.colmajor_min_bytes = v; }   // -1: never; 0: whenever the column-tile count allows
extern "C" void tpgsr_panel_set_enabled(int on) { g_conv_knobs.panel = on ? 1 : 0; }
extern "C" void tpgsr_panel_set_min_m(long long m) { g_conv_knobs.panel_min_m = m < 64 ? 64 : m; }
extern "C" void tpgsr_panel_set_k192(int on) { g_conv_knobs.panel_k192 = on ? 1 : 0; }
extern "C" void tpgsr_splitk_set_enabled(int on) { g_conv_knobs.splitk = on ? 1 : 0; }
extern "C" void tpgsr_wgrad3_set_enabled(int on) { g_conv_knobs.wgrad3 = on ? 1 : 0; }

// ---- predicates and geometry, each written once ----
int loader_bits(const tpgsr_conv_args* a) {
  return (a->in_scale ? 1 : 0) | (a->in_act ? 2 : 0) | (a->in2 ? 4 : 0) | (a->in_ps ? 8 : 0) | (a->in_b ? 16 : 0) | (a->in2_scale ? 32 : 0);
}

bool xbf_eligible(const tpgsr_conv_args* a) { return a->terms > 0 && a->wt_bf && (a->Cin & 3) == 0 && (a->wt_coff & 31) == 0; }

static int halo_capacity_of(const tpgsr_conv_args* a, int P) {   // P consecutive output pixels
  const int Wp = a->OW + a->KW - 1, ohw = a->OH * a->OW;
  const int row_wraps = (a->OW % P == 0) ? 0 : (P - 1) / a->OW + 1;
  const int img_wraps = (ohw % P == 0) ? 0 : (P - 1) / ohw + 1;
  return P - 1 + row_wraps * (a->KW - 1) + img_wraps * (a->KH - 1) * Wp + (a->KH - 1) * Wp + a->KW;
}
int halo_capacity(const tpgsr_conv_args* a) { return halo_capacity_of(a, 64); }
int halo3_capacity(const tpgsr_conv_args* a) { return halo_capacity_of(a, 64 * kH3Tiles); }

void wgrad_plan(long long M, int K, int Cout, int* Z, int* MB) {
  const int kb = cdiv(K, kWgradWK), nb = cdiv(Cout, kConvBN);
  // ~4 blocks per CU (TPGSR_WGRAD_TARGET: experiment switch -- fewer, longer splits write fewer slabs for the reduce to read back)
  long long z = (g_conv_knobs.wgrad_target + (long long)kb * nb - 1) / ((long long)kb * nb);
  long long maxz = (M + 255) / 256;  // at least 256 pixels per split
  if (maxz > 256) maxz = 256;
  if (z > maxz) z = maxz;
  if (z < 1) z = 1;
  long long mb = (M + z - 1) / z;
  mb = (mb + kWgradWM - 1) / kWgradWM * kWgradWM;      // whole staged chunks
  z = (M + mb - 1) / mb;
  *Z = (int)z;
  *MB = (int)mb;
}

// launches with fewer tiles than ~2/3 of the CUs and >= 24 K chunks: S workgroups per tile so that ~640 are resident, >= 6 chunks each
int splitk_choice(long long M, int Cout, int kp) {
  const ConvKnobs& k = g_conv_knobs;
  const long long ntiles = cdiv(M, 64) * cdiv(Cout, 64);
  const int nchunks = kp / kConvKC;
  if (ntiles > k.splitk_max_tiles || nchunks < k.splitk_min_k) return 0;
  int S = (int)(k.splitk_target / ntiles);
  S = S < 2 ? 2 : S > 8 ? 8 : S;
  int cps = (nchunks + S - 1) / S;
  if (cps < k.splitk_min_chunks) cps = k.splitk_min_chunks;
  S = (nchunks + cps - 1) / cps;          // no empty split
  return S > 1 ? S : 0;
}

// the loader variants each kernel is instantiated for (the T / loader-bits macros next to the kernels), as bit sets over ld
static constexpr unsigned long long ld_set(std::initializer_list<int> lds) {
  unsigned long long m = 0;
  for (int b : lds) m |= 1ull << b;
  return m;
}
static bool ld_in(int ld, unsigned long long set) { return (unsigned)ld < 64 && ((set >> ld) & 1); }
static constexpr unsigned long long kF32FwdLd = ld_set({0, 1, 2, 3, 4, 5, 7, 8, 17});
static constexpr unsigned long long kWgradTileLd = ld_set({0, 1, 2, 3, 4, 5, 7, 17});      // fp32 and split-bf16 tile loops alike
static constexpr unsigned long long kXbfFwdLd = ld_set({0, 1, 2, 3, 4, 5, 7, 8, 17});      // XBF_LD_CASES
static constexpr unsigned long long kHaloLd = ld_set({0, 1, 2, 3, 4, 5, 7});               // XBF_HALO_LD_CASES (the forward kernel adds 8)
static constexpr unsigned long long kHalo3Ld = ld_set({0, 1, 2, 3, 4, 5, 7, 37});          // H3_LD_CASES
static constexpr unsigned long long kPanelLd = ld_set({0, 1, 4, 17});                      // PANEL_LD_CASES
static constexpr unsigned long long kWgradBatchLd = ld_set({0, 1, 3});                     // XBF_WGB_CASE (tpgsr_conv_wgrad_batch)
bool wgrad_batch_has_ld(int ld) { return ld_in(ld, kWgradBatchLd); }

// ---- forward / data gradient ----
// whole-CU halo kernel: the halo capacity when the launch is its own, else 0
static int halo3_takes(const tpgsr_conv_args* a, long long M, int ld, int* lds_out) {
  const ConvKnobs& k = g_conv_knobs;
  const int T = a->terms, taps = a->KH * a->KW;
  if (!k.halo3 || T < 1 || T > 2 || taps < 3 || !(taps & 1) || a->wt_bf_cin != a->Cin || (a->Cin & 31) || a->stride_w > 1 || a->in_dil_w > 1 ||
      a->in_b || a->in_ps || !ld_in(ld, kHalo3Ld) || a->OW + a->KW - 1 < 8)
    return 0;
  // the residual-add loader carries two quads per entry and has ONE register set (no load of the next block in flight), and a
  // pixel-shuffled store goes out four bytes at a time: with both (the up-sampling convolution: 102 us here, 87 us there) the
  // two-workgroup kernel, whose second workgroup covers those waits, is faster
  if ((ld & 4) && a->out_ps) return 0;
  const int Lcap = halo3_capacity(a);
  const int lds = 2 * T * (32 * kH3Entries * 64) + 2 * kH3Tiles * 1024 + 8 * 4096;      // halo buffers + statistics scratch + epilogue staging (161 792 B at T = 2)
  if (Lcap > 32 * kH3Entries || lds > 163840) return 0;
  // one round of the chip (or several full ones): with fewer super-tiles than CUs the two-workgroup kernel spreads the work better
  const long long nst = (long long)cdiv(cdiv(M, 64), kH3Tiles) * cdiv(a->Cout, 64);
  if (nst < k.halo3_min_supertiles) return 0;
  *lds_out = lds;
  return Lcap;
}

// two-workgroup halo kernel: the halo capacity when the launch is its own, else 0
static int halo_takes(const tpgsr_conv_args* a, int ld, int* lds_out) {
  const ConvKnobs& k = g_conv_knobs;
  const int taps = a->KH * a->KW;
  if (!k.halo || taps < k.halo_min_taps || (a->wt_bf_cin != a->Cin && !(taps == 1 && a->wt_bf_cin == 0)) || (a->Cin & 31) || a->stride_w > 1 ||
      a->in_dil_w > 1 || a->in_b || !(ld_in(ld, kHaloLd) || ld == 8) || a->OW + a->KW - 1 < 8)
    return 0;
  const int Lcap = halo_capacity(a);
  const long long lds = 2ll * a->terms * Lcap * 64 + 2048;      // two halo buffers + two 1 KB statistics scratch areas
  // two workgroups per CU or not at all: with one, nothing covers a workgroup's barriers and epilogues (the 16x50 recognizer
  // conv, 278 halo entries = 107 KB in x3 mode, measured 54 us here against 47 us on the tile loop); seven entries per producer thread
  if (Lcap > 32 * 7 || lds > 80 * 1024) return 0;
  *lds_out = (int)lds;
  return Lcap;
}

// row-panel kernel: 32-column blocks per wave when the launch is its own, else 0
static int panel_takes(const tpgsr_conv_args* a, long long M, int ld, int* lds_out) {
  const ConvKnobs& k = g_conv_knobs;
  const int T = a->terms;
  if (!k.panel || a->KH * a->KW != 1 || a->wt_bf_cin != 0 || a->stride_w > 1 || a->in_dil_w > 1 || a->in_ps || a->pad_h || a->pad_w ||
      a->OH != a->H || a->OW != a->W || M < k.panel_min_m || T < 1 || T > 3)
    return 0;
  // (K / 32, 32-column blocks per wave) pairs instantiated: 64 -> <= 192, 96 -> <= 192, 192 -> <= 64
  const int nb32 = (a->Cout + 31) >> 5, nq8 = a->kp >> 5;
  int nbw = 0;
  if ((nq8 == 2 || nq8 == 3) && nb32 <= 6) nbw = 3;
  else if (nq8 == 6 && nb32 <= 2 && k.panel_k192) nbw = 1;
  else return 0;
  if (!ld_in(ld, kPanelLd)) return 0;
  const int panel = T * 64 * (nq8 * 64 + 16), epilogue = (4 * 64 * nbw + 4 * 1024) * 4;      // (epilogue scratch: statistics + staging)
  *lds_out = panel > epilogue ? panel : epilogue;
  return nbw;
}

static bool wstat_takes(const tpgsr_conv_args* a, int ld) {
  return g_conv_knobs.wstat && ld == 0 && a->KH == 3 && a->KW == 3 && a->pad_h == 1 && a->pad_w == 1 && a->Cin == 64 && a->Cout == 64 &&
         a->W == 64 && a->OW == 64 && a->OH == a->H && a->in_dil_w <= 1 && a->stride_w <= 1 && !a->out_ps && a->out_act == TPGSR_ACT_NONE &&
         (a->wt_ld == 0 || a->wt_ld == 64) && a->wt_coff == 0 && (a->in_ld & 3) == 0 && (a->in_coff & 3) == 0 &&
         (((uintptr_t)a->in | (uintptr_t)a->wt) & 15) == 0;
}

static tpgsr_conv_route_t fwd_route(const tpgsr_conv_args* a, long long M, int ld, bool planning) {
  tpgsr_conv_route_t r = {};
  r.ld = ld;
  if (!xbf_eligible(a)) {
    const int wld = a->wt_ld > 0 ? a->wt_ld : a->Cout;      // rows padded to a multiple of 4 floats
    const bool vecB = (wld & 3) == 0 && ((uintptr_t)a->wt & 15) == 0 && (a->wt_coff & 3) == 0;
    if (wstat_takes(a, ld)) {
      r.kernel = TPGSR_CONV_F32_WSTAT;
      r.lds_bytes = kWstatLdsBytes;
    } else if ((a->Cin & 3) != 0 || !vecB) {
      r.kernel = TPGSR_CONV_F32_SCALAR;
    } else {
      r.kernel = ld_in(ld, kF32FwdLd) ? TPGSR_CONV_F32_TILE : TPGSR_CONV_NONE;
    }
    return r;
  }
  if (!planning && a->sk_splits > 1) {      // the caller's split count wins over every other kernel
    r.kernel = ld_in(ld, kXbfFwdLd) ? TPGSR_CONV_XBF_SPLITK : TPGSR_CONV_NONE;
    r.splits = r.kernel ? a->sk_splits : 0;
    return r;
  }
  if ((r.lcap = halo3_takes(a, M, ld, &r.lds_bytes)) > 0) r.kernel = TPGSR_CONV_XBF_HALO3;
  else if ((r.lcap = halo_takes(a, ld, &r.lds_bytes)) > 0) r.kernel = TPGSR_CONV_XBF_HALO;
  else if ((r.nbw = panel_takes(a, M, ld, &r.lds_bytes)) > 0) r.kernel = TPGSR_CONV_XBF_PANEL;
  else r.kernel = ld_in(ld, kXbfFwdLd) ? TPGSR_CONV_XBF_TILE : TPGSR_CONV_NONE;
  // (planners only: the launcher has no use for it.)  Split-K is proposed for the tile loop's launches, and for the two-workgroup halo
  // kernel's all the same (conv6, 2 x 2 over 1248 pixels: 36.7 -> 31.3 us in x3, 28.9 -> 23.5 in x2) unless TPGSR_XBF_SPLITK_OVER_HALO=0
  // or the panel kernel would have taken the launch too
  int unused = 0;
  const ConvKnobs& k = g_conv_knobs;
  if (planning && k.splitk && a->terms <= 3 && a->bn_row_tiles <= 1 && !a->in2_scale && ld_in(ld, kXbfFwdLd) &&
      (r.kernel == TPGSR_CONV_XBF_TILE || (r.kernel == TPGSR_CONV_XBF_HALO && k.splitk_over_halo && !panel_takes(a, M, ld, &unused))))
    r.sk_plan = splitk_choice(M, a->Cout, a->kp);
  return r;
}

tpgsr_conv_route_t conv_fwd_route(const tpgsr_conv_args* a, long long M) { return fwd_route(a, M, loader_bits(a), false); }
tpgsr_conv_route_t conv_fwd_plan_route(const tpgsr_conv_args* a, long long M, int ld) { return fwd_route(a, M, ld, true); }

// ---- weight gradient ----
// geometry of the halo weight-gradient kernel, shared by its plan and the route
static bool wgrad_halo_shape_ok(const tpgsr_conv_args* a, int* Lcap_out) {
  const int taps = a->KH * a->KW;
  // only where it pays (TPGSR_XBF_WGRAD_HALO_MINWORK overrides the Cin x Cout threshold): measured at batch 48, the recognizer's
  // 128..512-channel convolutions and the 64->256 upsample convolution gain 15-30 % over the tile loop (conv5 225 -> 157 us,
  // upsample 156 -> 121 us) while the 64->64 trunk and 64->128 convolutions lose (42 -> 45 us: two channel blocks x 128 pixel
  // splits, every workgroup writes a slab for six tiles of work, plus the dy pre-split) and the whole C3 step came out 1 % slower
  // with them on -- profiles/r02b_wgrad_halo.md
  if ((long long)a->Cin * a->Cout < g_conv_knobs.wgrad_halo_minwork) return false;
  if (taps < 2 || taps > 12 || (a->Cin & 31) || a->stride_w > 1 || a->in_dil_w > 1 || a->in_ps || a->in_b || a->OW + a->KW - 1 < 8) return false;
  const int Lcap = halo_capacity(a);
  if (Lcap > 32 * 9) return false;
  *Lcap_out = Lcap;
  return true;
}

int wgrad_halo_plan(const tpgsr_conv_args* a, int cus, int* zsplits, long long* dy_bf_bytes) {
  int Lcap = 0;
  if (!g_conv_knobs.wgrad_halo || a->terms <= 0 || !wgrad_halo_shape_ok(a, &Lcap)) return 0;
  const long long M = (long long)a->N * a->OH * a->OW;
  const int tiles = cdiv(M, 64);
  const int groups = (a->Cin >> 5) * cdiv(a->Cout, 64);
  int Z = cus / groups;                                   // one workgroup per CU
  if (Z < 1) Z = 1;
  if (Z > tiles) Z = tiles;
  const int tpz = cdiv(tiles, Z);
  Z = cdiv(tiles, tpz);
  if (zsplits) *zsplits = Z;
  if (dy_bf_bytes) *dy_bf_bytes = 3ll * cdiv(M, 16) * cdiv(a->Cout, 32) * 1024;
  return 1;
}

tpgsr_wgrad_route_t conv_wgrad_route(const tpgsr_wgrad_args* w, long long M) {
  const tpgsr_conv_args* a = &w->c;
  const int K = a->KH * a->KW * a->Cin, T = a->terms;
  tpgsr_wgrad_route_t r = {};
  const int ld = r.ld = loader_bits(a);
  wgrad_plan(M, K, a->Cout, &r.Z, &r.MB);
  if (w->zsplits > 0) {   // the caller's split count: whole 64-pixel tiles per split (what the halo kernel walks)
    r.Z = w->zsplits;
    r.MB = cdiv(cdiv(M, 64), r.Z) * 64;
  }
  // rows padded to a multiple of 4 floats keep an odd channel count (the 37 classes) on the vector path: the loads of the
  // last quad stay inside the padded row, columns >= Cout are never stored
  r.vecY = (!w->dy_ps && (w->dy_ld & 3) == 0 && (w->dy_coff & 3) == 0 && w->dy_ld >= ((a->Cout + 3) & ~3) + w->dy_coff &&
            ((uintptr_t)w->dy & 15) == 0) ? 1 : 0;
  if (!(T > 0 && (a->Cin & 3) == 0 && (r.vecY || w->dy_ps))) {
    if ((a->Cin & 3) != 0 || (!r.vecY && !w->dy_ps)) r.kernel = TPGSR_WGRAD_F32_SCALAR;
    else r.kernel = ld_in(ld, kWgradTileLd) ? TPGSR_WGRAD_F32_TILE : TPGSR_WGRAD_NONE;
    return r;
  }
  int Lcap = 0;
  if (g_conv_knobs.wgrad_halo && w->zsplits > 0 && w->dy_bf && ld_in(ld, kHaloLd) && wgrad_halo_shape_ok(a, &Lcap) &&
      2ll * T * Lcap * 64 + 512 <= 150 * 1024) {
    r.kernel = TPGSR_WGRAD_XBF_HALO;
    r.lcap = Lcap;
    r.ne = Lcap <= 32 * 7 ? 7 : 9;
    r.lds_bytes = 2 * T * Lcap * 64 + 512;
  } else if (g_conv_knobs.wgrad3 && T <= 2 && K % (3 * kWgradWK) == 0 && (ld == 0 || ld == 1) && !w->dy_ps && a->in_dil_w <= 1 && a->stride_w <= 1 &&
             !a->in_ps && M * (long long)w->dy_ld * 4 <= 0x7fffffffll) {
    // three k-blocks per workgroup where the shape allows: K a multiple of 192, the plain / affine loader, dense dy, a plain stride-1 geometry
    r.kernel = TPGSR_WGRAD_XBF_3K;
  } else {
    r.kernel = ld_in(ld, kWgradTileLd) ? TPGSR_WGRAD_XBF_TILE : TPGSR_WGRAD_NONE;
  }
  return r;
}

// ---- C ABI: the route itself, and the planners over it ----
static long long pixels(const tpgsr_conv_args* a) { return (long long)a->N * a->OH * a->OW; }
// (the launchers validate before they route; the exported route divides by these as well)
static bool geometry_ok(const tpgsr_conv_args* a) { return a->N > 0 && a->OH > 0 && a->OW > 0 && a->Cin > 0 && a->Cout > 0 && a->KH > 0 && a->KW > 0; }

extern "C" int tpgsr_conv_route(const tpgsr_conv_args* a, tpgsr_conv_route_t* r) {
  if (!a || !r || !geometry_ok(a)) return -1;
  *r = conv_fwd_route(a, pixels(a));
  r->sk_plan = conv_fwd_plan_route(a, pixels(a), r->ld).sk_plan;
  return r->kernel;
}

extern "C" int tpgsr_conv_wgrad_route(const tpgsr_wgrad_args* w, tpgsr_wgrad_route_t* r) {
  if (!w || !r || !geometry_ok(&w->c)) return -1;
  *r = conv_wgrad_route(w, pixels(&w->c));
  return r->kernel;
}

extern "C" int tpgsr_halo_capacity(const tpgsr_conv_args* a) { return a ? halo_capacity(a) : -1; }   // (tests/test_halo_host_cpu.py)

extern "C" int tpgsr_wgrad_splits(int M, int K, int Cout) {
  int Z, MB;
  wgrad_plan(M, K, Cout, &Z, &MB);
  return Z;
}

extern "C" int tpgsr_conv_splitk_plan(const tpgsr_conv_args* a, long long* bytes) {
  if (bytes) *bytes = 0;
  if (!a || !xbf_eligible(a)) return 0;
  const long long M = pixels(a);
  const int S = conv_fwd_plan_route(a, M, loader_bits(a) & ~32).sk_plan;      // (a launch with in2_scale is never split: the route says 0)
  if (S > 1 && bytes) *bytes = (long long)S * cdiv(M, 64) * cdiv(a->Cout, 64) * 256 * 16 * 4;
  return S;
}

/* 1 when a launch with a scaled residual operand (tpgsr_conv_args.in2_scale) is the whole-CU halo kernel's -- the only one whose loader has it */
extern "C" int tpgsr_conv_in2_scale_ok(const tpgsr_conv_args* a) {
  if (!a || !xbf_eligible(a) || !a->in2 || !a->in_scale || a->in_act || a->in_b) return 0;
  return conv_fwd_plan_route(a, pixels(a), 37).kernel == TPGSR_CONV_XBF_HALO3 ? 1 : 0;
}

/* tpgsr_conv_args.bn_row_tiles: 3 when tpgsr_conv_fwd(a) lands on the whole-CU halo kernel (asked before in2_scale is set: bit 32 masked) */
extern "C" int tpgsr_conv_bn_row_tiles(const tpgsr_conv_args* a) {
  if (!a || !xbf_eligible(a)) return 1;
  return conv_fwd_plan_route(a, pixels(a), loader_bits(a) & ~32).kernel == TPGSR_CONV_XBF_HALO3 ? kH3Tiles : 1;
}
