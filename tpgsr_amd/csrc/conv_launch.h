// The per-kernel launchers behind tpgsr_conv_fwd / tpgsr_conv_wgrad (conv_mfma.hip): each takes the route the caller computed
// (conv_route.h) and returns 0 or an error code.
#pragma once
#include "common.h"
#include "conv_route.h"
#pragma GCC visibility push(hidden)

// opt-in to > 64 KB of dynamic LDS, per (kernel, device): raised to the largest size seen so far.  No-op up to 64 KB.
int lds_opt_in(const void* fn, size_t bytes, const char* who);
// (a route whose loader variant the launcher's instantiation table does not have: the two lists disagree)
int unsupported_ld(const char* who, int ld);

int conv_fwd_xbf_launch(const tpgsr_conv_args* a, long long M, int K, const tpgsr_conv_route_t& r, hipStream_t st);     // split-K, tile loop
int conv_halo_xbf_launch(const tpgsr_conv_args* a, long long M, const tpgsr_conv_route_t& r, hipStream_t st);
int conv_halo3_xbf_launch(const tpgsr_conv_args* a, long long M, const tpgsr_conv_route_t& r, hipStream_t st);
int conv_panel_xbf_launch(const tpgsr_conv_args* a, long long M, const tpgsr_conv_route_t& r, hipStream_t st);
int conv_wgrad_xbf_launch(const tpgsr_wgrad_args* w, long long M, int K, const tpgsr_wgrad_route_t& r, hipStream_t st);  // three k-blocks, tile loop
int conv_wgrad_halo_launch(const tpgsr_wgrad_args* w, long long M, const tpgsr_wgrad_route_t& r, hipStream_t st);
#pragma GCC visibility pop
