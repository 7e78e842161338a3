// Stand-alone check that the convolution route (tpgsr_amd/csrc/conv_route.cpp) is a pure host function: this program links that one
// translation unit -- no HIP, no Python, no device -- and walks the geometry of tests/golden/make_golden_routes.py's sweep under the
// host sanitizers.  From the repository root:
//
//   c++ -std=c++20 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/conv_route_check.cpp tpgsr_amd/csrc/conv_route.cpp \
//       -o /tmp/conv_route_check && /tmp/conv_route_check
//
// Every argument block sits at the END of its own heap allocation (a read past the struct is an AddressSanitizer report) and is compared
// byte for byte after the calls (the route writes nothing).  Invariants checked for every case: the launch parameters stay inside what
// the kernels are built for, a second call gives the same answer, and the planners agree with the launch they plan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>

#include "../tpgsr_amd/csrc/conv_route.h"

static long long failures = 0, cases = 0;
static int seen_fwd[9], seen_wg[6];
#define EXPECT(cond, ...)                                 \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) {                              \
        fprintf(stderr, "FAILED %s: ", #cond);            \
        fprintf(stderr, __VA_ARGS__);                     \
        fputc('\n', stderr);                              \
      }                                                   \
    }                                                     \
  } while (0)

static char dummy[4096] __attribute__((aligned(16)));      // operand addresses: only their alignment is ever looked at

static void check_fwd(const tpgsr_conv_args& proto) {
  std::unique_ptr<char[]> mem(new char[sizeof(tpgsr_conv_args)]);       // exactly the struct: the allocation ends where it ends
  tpgsr_conv_args* a = reinterpret_cast<tpgsr_conv_args*>(mem.get());
  memcpy(a, &proto, sizeof(*a));
  const long long M = (long long)a->N * a->OH * a->OW;
  tpgsr_conv_route_t r, r2;
  const int k = tpgsr_conv_route(a, &r);
  tpgsr_conv_route(a, &r2);
  ++cases;
  EXPECT(k == r.kernel && k >= 0 && k <= TPGSR_CONV_XBF_TILE, "kernel %d", k);
  if (k >= 0 && k <= TPGSR_CONV_XBF_TILE) seen_fwd[k]++;
  EXPECT(memcmp(&r, &r2, sizeof(r)) == 0, "two calls differ");
  EXPECT(memcmp(a, &proto, sizeof(*a)) == 0, "the argument block was written");
  EXPECT(r.ld == loader_bits(a), "ld %d", r.ld);
  EXPECT(r.lds_bytes >= 0 && r.lds_bytes <= 160 * 1024, "lds %d", r.lds_bytes);
  EXPECT((k >= TPGSR_CONV_XBF_SPLITK) <= xbf_eligible(a), "a split-bf16 kernel for an fp32 launch");
  if (k == TPGSR_CONV_XBF_HALO) EXPECT(r.lcap == halo_capacity(a) && r.lcap <= 32 * 7 && r.lds_bytes == 2 * a->terms * r.lcap * 64 + 2048 && r.lds_bytes <= 80 * 1024, "halo lcap %d lds %d", r.lcap, r.lds_bytes);
  if (k == TPGSR_CONV_XBF_HALO3) EXPECT(r.lcap == halo3_capacity(a) && r.lcap <= 32 * kH3Entries && a->terms <= 2, "halo3 lcap %d", r.lcap);
  if (k == TPGSR_CONV_XBF_PANEL) EXPECT((r.nbw == 3 || r.nbw == 1) && a->KH * a->KW == 1 && r.lds_bytes >= a->terms * 64 * a->kp * 2, "panel nbw %d lds %d", r.nbw, r.lds_bytes);
  if (k == TPGSR_CONV_XBF_SPLITK) EXPECT(r.splits == a->sk_splits && r.splits > 1, "splits %d", r.splits);
  if (k == TPGSR_CONV_F32_WSTAT) EXPECT(r.lds_bytes == kWstatLdsBytes && M % 64 == 0, "wstat");
  // planners
  long long bytes = -1;
  const int S = tpgsr_conv_splitk_plan(a, &bytes);
  EXPECT(S == r.sk_plan && S != 1 && S <= 8 && (S > 1) == (bytes > 0), "split-K plan %d, route %d, %lld bytes", S, r.sk_plan, bytes);
  if (S > 1) {
    EXPECT(S <= a->kp / 32, "more splits (%d) than K chunks (%d)", S, a->kp / 32);
    tpgsr_conv_args b = *a;
    b.sk_splits = S;
    tpgsr_conv_route_t rb;
    EXPECT(tpgsr_conv_route(&b, &rb) == TPGSR_CONV_XBF_SPLITK && rb.splits == S, "the proposal is not what the launcher runs");
  }
  if (a->sk_splits <= 1) {
    const bool h3 = k == TPGSR_CONV_XBF_HALO3;
    if (!a->in2_scale) EXPECT(tpgsr_conv_bn_row_tiles(a) == (h3 ? kH3Tiles : 1), "bn_row_tiles");
    else EXPECT(tpgsr_conv_in2_scale_ok(a) == (h3 ? 1 : 0), "in2_scale_ok");
  }
}

static void check_wgrad(const tpgsr_wgrad_args& proto) {
  std::unique_ptr<char[]> mem(new char[sizeof(tpgsr_wgrad_args)]);
  tpgsr_wgrad_args* w = reinterpret_cast<tpgsr_wgrad_args*>(mem.get());
  memcpy(w, &proto, sizeof(*w));
  const tpgsr_conv_args* a = &w->c;
  const long long M = (long long)a->N * a->OH * a->OW;
  tpgsr_wgrad_route_t r, r2;
  const int k = tpgsr_conv_wgrad_route(w, &r);
  tpgsr_conv_wgrad_route(w, &r2);
  ++cases;
  EXPECT(k == r.kernel && k >= 0 && k <= TPGSR_WGRAD_XBF_TILE, "kernel %d", k);
  if (k >= 0 && k <= TPGSR_WGRAD_XBF_TILE) seen_wg[k]++;
  EXPECT(memcmp(&r, &r2, sizeof(r)) == 0, "two calls differ");
  EXPECT(memcmp(w, &proto, sizeof(*w)) == 0, "the argument block was written");
  EXPECT(r.Z >= 1 && r.MB >= 1 && (long long)r.Z * r.MB >= M, "Z %d x MB %d does not cover M %lld", r.Z, r.MB, M);
  EXPECT(w->zsplits > 0 ? (r.Z == w->zsplits && r.MB % 64 == 0) : (r.Z == tpgsr_wgrad_splits((int)M, a->KH * a->KW * a->Cin, a->Cout) && r.MB % 32 == 0), "Z %d MB %d", r.Z, r.MB);
  int z = 0;
  long long nb = 0;
  const int plan = wgrad_halo_plan(a, 256, &z, &nb);
  if (k == TPGSR_WGRAD_XBF_HALO) {
    EXPECT(plan == 1 && r.lcap == halo_capacity(a) && r.lcap <= 32 * r.ne && (r.ne == 7 || r.ne == 9) && r.lds_bytes <= 150 * 1024 && w->dy_bf, "halo lcap %d ne %d", r.lcap, r.ne);
    EXPECT(nb >= 2ll * 3 * ((M + 15) / 16) * ((a->Cout + 31) / 32) * 512, "dy_bf scratch of %lld bytes", nb);
  }
  if (plan) EXPECT(z >= 1 && z <= (M + 63) / 64 && (long long)z * (a->Cin >> 5) * ((a->Cout + 63) / 64) <= 256 + (a->Cin >> 5) * ((a->Cout + 63) / 64), "halo plan Z %d", z);
  if (k == TPGSR_WGRAD_XBF_3K) EXPECT(a->KH * a->KW * a->Cin % 192 == 0 && a->terms <= 2, "three k-blocks");
}

int main() {
  const int taps[][4] = {{1, 1, 0, 0}, {2, 2, 0, 0}, {3, 3, 1, 1}, {9, 9, 4, 4}, {1, 3, 0, 1}};
  const int ows[] = {6, 7, 8, 16, 26, 50, 64, 65, 128}, chans[] = {4, 32, 37, 64, 96, 128, 192, 256, 512};
  const int lds[] = {0, 1, 2, 3, 4, 5, 7, 8, 17, 37, 6, 16, 33};
  for (const auto& t : taps)
    for (int OW : ows)
      for (int Ci : chans)
        for (int Co : chans)
          for (int terms = 0; terms <= 3; ++terms)
            for (int N : {1, 2, 48, 97})
              for (int ld : lds) {
                tpgsr_conv_args a;
                memset(&a, 0, sizeof(a));
                a.in = reinterpret_cast<const float*>(dummy);
                a.wt = reinterpret_cast<const float*>(dummy + 64);
                a.out = reinterpret_cast<float*>(dummy + 128);
                a.N = N, a.H = t[0] > 3 ? 12 : 16, a.W = OW, a.Cin = Ci, a.Cout = Co, a.KH = t[0], a.KW = t[1], a.pad_h = t[2], a.pad_w = t[3];
                a.OH = a.H + 2 * a.pad_h - a.KH + 1, a.OW = a.W + 2 * a.pad_w - a.KW + 1;
                a.in_ld = a.in2_ld = Ci, a.out_ld = Co, a.in_dil_w = a.stride_w = 1;
                if (ld & 1) a.in_scale = a.in_shift = reinterpret_cast<const float*>(dummy + 256);
                if (ld & 2) a.in_act = TPGSR_ACT_MISH;
                if (ld & 4) a.in2 = reinterpret_cast<const float*>(dummy + 512);
                if (ld & 8) a.in_ps = 1;
                if (ld & 16) a.in_b = reinterpret_cast<const float*>(dummy + 768), a.cin_a = Ci / 2, a.in_b_ld = Ci - Ci / 2;
                if (ld & 32) a.in2_scale = reinterpret_cast<const float*>(dummy + 1024);
                a.terms = terms;
                if (terms && Ci % 4 == 0) {
                  a.kp = (a.KH * a.KW * Ci + 31) / 32 * 32;
                  a.wt_bf = dummy + 2048;
                  a.wt_bf_cin = (Ci % 32 == 0 && a.KH * a.KW > 1) ? Ci : 0;
                }
                check_fwd(a);
                if (ld == 0 && N == 48) {
                  tpgsr_conv_args b = a;
                  b.sk_splits = 4, b.sk_part = reinterpret_cast<float*>(dummy + 3072);
                  check_fwd(b);
                  b = a, b.out_ps = 1;
                  check_fwd(b);
                  b = a, b.stride_w = 2;
                  check_fwd(b);
                  b = a, b.wt = reinterpret_cast<const float*>(dummy + 68);
                  check_fwd(b);
                }
                if (ld & 32) continue;
                tpgsr_wgrad_args w;
                memset(&w, 0, sizeof(w));
                w.c = a;
                w.dy = reinterpret_cast<const float*>(dummy + 1536), w.part = reinterpret_cast<float*>(dummy + 1792);
                w.dy_ld = (Co + 3) / 4 * 4;
                check_wgrad(w);
                w.zsplits = 8, w.dy_bf = dummy + 2560;
                check_wgrad(w);
                if (ld == 0) {
                  w.dy_ld = Co, w.dy = reinterpret_cast<const float*>(dummy + 1540);
                  check_wgrad(w);
                  if (Co % 4 == 0) {
                    w.dy_ps = 1;
                    check_wgrad(w);
                  }
                }
              }
  for (int k = 0; k <= TPGSR_CONV_XBF_TILE; ++k) EXPECT(seen_fwd[k] > 0, "forward kernel %d never chosen", k);
  for (int k = 0; k <= TPGSR_WGRAD_XBF_TILE; ++k) EXPECT(seen_wg[k] > 0, "weight-gradient kernel %d never chosen", k);
  printf("%lld cases, %lld failures\n", cases, failures);
  return failures ? 1 : 0;
}
