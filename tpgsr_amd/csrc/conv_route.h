// Which kernel a convolution launch runs on: ONE host-side decision, shared by the launchers (tpgsr_conv_fwd / tpgsr_conv_wgrad)
// and by every planner that sizes a buffer or picks an argument for the kernel the launcher is going to choose
// (tpgsr_conv_splitk_plan, tpgsr_conv_bn_row_tiles, tpgsr_conv_in2_scale_ok, tpgsr_wgrad_halo_plan, tpgsr_conv_wgrad_batch_prepare).
// Host only: no device code, no HIP call, no getenv / allocation / lock per call -- a pure function of the argument block and ConvKnobs
// (tools/conv_route_check.cpp links conv_route.cpp alone).
#pragma once
#include "../../include/tpgsr_hip.h"
#pragma GCC visibility push(hidden)   // internal to the library: only the C ABI is exported

// every switch the route (and the launchers' host side) reads: initialised once from the environment when the library is loaded, written
// by the tpgsr_*_set_* entry points
struct ConvKnobs {
  int wstat;                       // TPGSR_CONV_WSTAT (1): weights-stationary fp32 kernel for the 64-channel 3x3 trunk on 64-wide maps
  long long wgrad_target;          // TPGSR_WGRAD_TARGET (1024): workgroups a tile-loop weight gradient aims at
  int halo3;                       // TPGSR_XBF_HALO3 (1) / tpgsr_halo3_set_enabled
  long long halo3_min_supertiles;  // TPGSR_XBF_HALO3_MIN (192)
  int halo;                        // TPGSR_XBF_HALO (1)
  int halo_min_taps;               // TPGSR_XBF_HALO_MINTAPS (2; 1 takes 1x1 convolutions as well) / tpgsr_halo_set_min_taps
  long long colmajor_min_bytes;    // (3 MB) / tpgsr_halo_set_colmajor_min_bytes: weight planes above which the halo kernel walks tiles column-major
  int panel;                       // TPGSR_XBF_PANEL (1) / tpgsr_panel_set_enabled
  long long panel_min_m;           // TPGSR_XBF_PANEL_MIN_M (32768) / tpgsr_panel_set_min_m
  int panel_k192;                  // TPGSR_XBF_PANEL_K192 (0) / tpgsr_panel_set_k192
  int splitk;                      // TPGSR_XBF_SPLITK (1) / tpgsr_splitk_set_enabled
  int splitk_target, splitk_min_chunks, splitk_max_tiles, splitk_min_k;   // TPGSR_XBF_SPLITK_TARGET (640), _MIN_CHUNKS (6), _MAX_TILES (256), _MIN_K (24)
  int splitk_over_halo;            // TPGSR_XBF_SPLITK_OVER_HALO (1): split a launch the two-workgroup halo kernel would take all the same
  int wgrad3;                      // TPGSR_XBF_WGRAD3 (1) / tpgsr_wgrad3_set_enabled
  int wgrad_halo;                  // TPGSR_XBF_WGRAD_HALO (1)
  long long wgrad_halo_minwork;    // TPGSR_XBF_WGRAD_HALO_MINWORK (16384): Cin x Cout from which the halo weight-gradient kernel pays
};
extern ConvKnobs g_conv_knobs;

// tile constants the route shares with the kernels (each kernel file static_asserts its own macros against them)
constexpr int kConvKC = 32, kConvBN = 64;                                       // K chunk / channels per tile of every tile loop
constexpr int kWgradWK = 64, kWgradWM = 32;                                     // weight gradient: k rows per workgroup / pixels per staged chunk
constexpr int kH3Tiles = 3, kH3Entries = 15;                                   // whole-CU halo kernel: 64-pixel tiles / halo entries per producer thread
constexpr int kWstatLdsBytes = 4 * (9 * 32 * 64 + 3 * ((3 * 66 + 7) / 8 * 8) * 32);   // weights-stationary kernel: weight slice + three halos

// compile-time loader variant: 1 affine, 2 activation, 4 residual add, 8 pixel-shuffle gather, 16 concatenated strip, 32 scaled residual
int loader_bits(const tpgsr_conv_args* a);
// split-bf16 kernels (conv_xbf.hip, conv_halo3.hip, conv_panel.hip): vector loader + pre-split weights
bool xbf_eligible(const tpgsr_conv_args* a);

// upper bound of the halo length of any 64-pixel tile / any run of 192 consecutive output pixels
int halo_capacity(const tpgsr_conv_args* a);
int halo3_capacity(const tpgsr_conv_args* a);
// tile-loop weight gradient: pixel splits Z of MB pixels each
void wgrad_plan(long long M, int K, int Cout, int* Z, int* MB);
// split-K: workgroups per tile (0: do not split) for launches with few tiles and a long contraction
int splitk_choice(long long M, int Cout, int kp);
// halo weight-gradient kernel: 1 + (*zsplits, *dy_bf_bytes) when the geometry is its own, on a chip of `cus` compute units
int wgrad_halo_plan(const tpgsr_conv_args* a, int cus, int* zsplits, long long* dy_bf_bytes);

// M = N * OH * OW.  Tests in the launcher's order: explicit sk_splits, whole-CU halo, two-workgroup halo, panel, tile loop (split-bf16);
// weights-stationary, tile loop, scalar loader (fp32).  kernel = TPGSR_CONV_NONE: no kernel has this loader combination.
tpgsr_conv_route_t conv_fwd_route(const tpgsr_conv_args* a, long long M);
// the same for a planner: a->sk_splits is ignored (the planner is what proposes it: sk_plan is filled here only) and the loader variant is
// the caller's
tpgsr_conv_route_t conv_fwd_plan_route(const tpgsr_conv_args* a, long long M, int ld);
// halo, three-k-block, tile loop (split-bf16); tile loop, scalar loader (fp32)
tpgsr_wgrad_route_t conv_wgrad_route(const tpgsr_wgrad_args* w, long long M);
// the loader variants the batched weight-gradient kernel is instantiated for (a launch with another one goes out singly)
bool wgrad_batch_has_ld(int ld);
#pragma GCC visibility pop
