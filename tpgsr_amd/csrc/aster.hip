// ASTER evaluation recognizer, greedy and beam-search decode (reference model/recognizer/*, interfaces/base.py:844-864):
//   * parse_aster_data: bicubic resize of the RGB planes + [0,1] -> [-1,1], NCHW in, NHWC out (interfaces/base.py:852-858)
//   * one decoder step of AttentionRecognitionHead.sample (attention_recognition_head.py:47-67): attention weights + context
//     (AttentionUnit :196-218, DecoderUnit :258-260), embedding lookup + concat (:262-264), GRU cell gate math (nn.GRU, :264),
//     softmax arg-max + score (:60-61)
// The encoder (ResNet_ASTER + 2-layer BiLSTM), the STN head and the TPS rectification reuse the conv / BN / pool / LSTM / TPS kernels.
#include "common.h"

__device__ __forceinline__ void aster_cubic(float t, float (&w)[4]) {     // A = -0.75, as F.interpolate(mode='bicubic')
  const float A = -0.75f;
  float x = t + 1.f;
  w[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  x = t;
  w[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 1.f - t;
  w[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  x = 2.f - t;
  w[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}
__device__ __forceinline__ void aster_src(int o, int in_size, int out_size, int& i0, float (&w)[4]) {
  const float scale = (float)in_size / (float)out_size;
  const float x = ((float)o + 0.5f) * scale - 0.5f;
  const float fx = floorf(x);
  i0 = (int)fx;
  aster_cubic(x - fx, w);
}
__device__ __forceinline__ int aster_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// out[n][oh][ow][c] = scale * bicubic(in[n][c])(oh, ow) + shift,  c < C (the first C of Ctot planes), align_corners = False
__global__ __launch_bounds__(256) void bicubic_resize_kernel(const float* __restrict__ in, int N, int Ctot, int C, int H, int W, int OH,
                                                             int OW, float scale, float shift, float* __restrict__ out) {
  const long long total = (long long)N * OH * OW * C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  long long r = i / C;
  const int ow = (int)(r % OW);
  r /= OW;
  const int oh = (int)(r % OH), n = (int)(r / OH);
  int y0, x0;
  float wy[4], wx[4];
  aster_src(oh, H, OH, y0, wy);
  aster_src(ow, W, OW, x0, wx);
  const float* p = in + ((size_t)n * Ctot + c) * H * W;
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int yy = aster_clamp(y0 - 1 + a, H - 1);
    float rowv = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) rowv += p[(size_t)yy * W + aster_clamp(x0 - 1 + b, W - 1)] * wx[b];
    acc += rowv * wy[a];
  }
  out[i] = acc * scale + shift;
}

extern "C" int tpgsr_bicubic_resize(const float* in_nchw, int N, int Ctot, int C, int H, int W, int OH, int OW, float scale, float shift,
                                    float* out_nhwc, void* stream) {
  TPGSR_CHECK_ARG(in_nchw && out_nhwc && N > 0 && C > 0 && Ctot >= C && H > 0 && W > 0 && OH > 0 && OW > 0, "tpgsr_bicubic_resize: bad arguments");
  const long long total = (long long)N * OH * OW * C;
  hipLaunchKernelGGL(bicubic_resize_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, in_nchw, N, Ctot, C, H, W, OH, OW,
                     scale, shift, out_nhwc);
  TPGSR_LAUNCH_CHECK("tpgsr_bicubic_resize");
}

// ------------------------------------------------------------------------------------------------------
// `--arch bicubic` (model/bicubic.py): F.interpolate(x, scale_factor=s, mode='bicubic', align_corners=True) of the first C of Ctot
// NCHW planes, NCHW out.  One thread = BU_PX adjacent output pixels of one output row, for every channel: the column tap indices and
// their four weight quadruples are computed once and reused by all C planes and tap rows (the row's index and weight are re-derived
// per row from the row fraction: a few operations, against 64 live tap addresses); a thread's pixels go out as one 16-byte store where the row
// length and the pointer allow it (consecutive threads = consecutive 16-byte pieces of a row), scalar stores at ragged row ends.
// The source coordinate o * (in - 1) / (out - 1) is formed in integers (quotient = first tap, remainder / (out - 1) = fraction), so
// the fraction carries one rounding instead of the cancellation of floor() on a float product.
// ------------------------------------------------------------------------------------------------------
#define BU_PX 4
__device__ __forceinline__ float bu_src(int o, int in_size, int out_size, int& i0) {      // -> the tap fraction
  if (out_size <= 1) {
    i0 = 0;
    return 0.f;
  }
  const long long num = (long long)o * (in_size - 1);
  const int den = out_size - 1;
  i0 = (int)(num / den);
  return (float)(num - (long long)i0 * den) / (float)den;
}
__device__ __forceinline__ float bu_weight(float t, int a) {      // element a of aster_cubic(t, .)
  const float A = -0.75f;
  if (a == 1 || a == 2) {
    const float x = a == 1 ? t : 1.f - t;
    return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  }
  const float x = a == 0 ? t + 1.f : 2.f - t;
  return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

__global__ __launch_bounds__(256) void bicubic_upsample_kernel(const float* __restrict__ in, int N, int Ctot, int C, int H, int W, int OH,
                                                               int OW, float* __restrict__ out) {
  const int groups = (OW + BU_PX - 1) / BU_PX;
  const long long total = (long long)N * OH * groups;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int gx = (int)(i % groups);
  const long long r = i / groups;
  const int oh = (int)(r % OH), n = (int)(r / OH);
  const int ow0 = gx * BU_PX;
  int y0, xi[BU_PX][4];
  float wx[BU_PX][4];
  const float ty = bu_src(oh, H, OH, y0);
#pragma unroll
  for (int p = 0; p < BU_PX; ++p) {
    int x0;
    aster_cubic(bu_src(min(ow0 + p, OW - 1), W, OW, x0), wx[p]);      // (a pixel past the row end repeats the last one and is not stored)
#pragma unroll
    for (int b = 0; b < 4; ++b) xi[p][b] = aster_clamp(x0 - 1 + b, W - 1);
  }
  const bool vec = (OW % BU_PX) == 0;
  for (int c = 0; c < C; ++c) {
    const float* src = in + ((size_t)n * Ctot + c) * H * W;
    float acc[BU_PX];
#pragma unroll
    for (int p = 0; p < BU_PX; ++p) acc[p] = 0.f;
    // one tap row at a time: unrolled over the rows (and planes) the compiler keeps all 64 tap addresses of a thread live as 64-bit
    // pairs -- 228 VGPRs, two waves per SIMD; the row's weight and clamped index are a handful of wave-uniform-cost operations
#pragma unroll 1
    for (int a = 0; a < 4; ++a) {
      const float* row = src + (size_t)aster_clamp(y0 - 1 + a, H - 1) * W;
      const float wya = bu_weight(ty, a);
#pragma unroll
      for (int p = 0; p < BU_PX; ++p) {
        float rowv = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) rowv += row[xi[p][b]] * wx[p][b];
        acc[p] += rowv * wya;
      }
    }
    float* dst = out + (((size_t)n * C + c) * OH + oh) * OW + ow0;
    if (vec && (((uintptr_t)dst) & 15) == 0) {
      *reinterpret_cast<floatx4*>(dst) = floatx4{acc[0], acc[1], acc[2], acc[3]};
    } else {
#pragma unroll
      for (int p = 0; p < BU_PX; ++p)
        if (ow0 + p < OW) dst[p] = acc[p];
    }
  }
}

extern "C" int tpgsr_bicubic_upsample(const float* in_nchw, int N, int Ctot, int C, int H, int W, int scale, float* out_nchw, void* stream) {
  TPGSR_CHECK_ARG(in_nchw && out_nchw, "tpgsr_bicubic_upsample: null pointer");
  TPGSR_CHECK_ARG(N > 0 && H > 0 && W > 0, "tpgsr_bicubic_upsample: N, H and W must be at least 1 (got N %d, H %d, W %d)", N, H, W);
  TPGSR_CHECK_ARG(C >= 1 && C <= Ctot, "tpgsr_bicubic_upsample: reads the first C of Ctot planes, 1 <= C <= Ctot (got C %d, Ctot %d)", C, Ctot);
  TPGSR_CHECK_ARG(scale >= 1, "tpgsr_bicubic_upsample: the integer scale factor must be at least 1 (got %d)", scale);
  TPGSR_CHECK_ARG((long long)H * scale <= 0x7fffffffLL && (long long)W * scale <= 0x7fffffffLL,
                  "tpgsr_bicubic_upsample: H * scale and W * scale must stay below 2^31 (got H %d, W %d, scale %d)", H, W, scale);
  const int OH = H * scale, OW = W * scale;
  const long long total = (long long)N * OH * ((OW + BU_PX - 1) / BU_PX);
  TPGSR_CHECK_ARG(total <= 0x7fffffffLL * 256, "tpgsr_bicubic_upsample: N * OH * ceil(OW / %d) = %lld threads exceed the grid limit 2^31 * 256",
                  BU_PX, total);
  hipLaunchKernelGGL(bicubic_upsample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in_nchw, N, Ctot, C, H,
                     W, OH, OW, out_nchw);
  TPGSR_LAUNCH_CHECK("tpgsr_bicubic_upsample");
}

// ------------------------------------------------------------------------------------------------------
// attention of one decoder step, one workgroup per decoder row r; row r attends over sequence r / rows_per_seq (a beam decode keeps
// rows_per_seq beams per image on ONE copy of the image's features and their projection; the greedy decode has rows_per_seq = 1):
//   v[t] = wv . tanh(sproj[r] + xproj[q][t]) + bv;  alpha = softmax_t(v);  context[r] = sum_t alpha[t] x[q][t],   q = r / rows_per_seq
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aster_attention_kernel(const float* __restrict__ xproj, const float* __restrict__ sproj,
                                                              const float* __restrict__ wv, const float* __restrict__ bv,
                                                              const float* __restrict__ x, int rows_per_seq, int T, int A, int D,
                                                              float* __restrict__ alpha, float* __restrict__ context) {
  extern __shared__ float sm[];      // [T] scores
  const int n = blockIdx.x, q = n / rows_per_seq, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xp = xproj + (size_t)q * T * A;
  const float* sp = sproj + (size_t)n * A;
  for (int t = wave; t < T; t += 4) {           // one wave per time step, lanes over the attention dimension
    float acc = 0.f;
    for (int a = lane; a < A; a += 64) acc += wv[a] * tanh_f(sp[a] + xp[(size_t)t * A + a]);
    acc = wave_sum(acc);
    if (lane == 0) sm[t] = acc + bv[0];
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int t = 0; t < T; ++t) mx = fmaxf(mx, sm[t]);
  float den = 0.f;
  for (int t = 0; t < T; ++t) den += expf(sm[t] - mx);
  const float inv = 1.f / den;
  if (tid < T) alpha[(size_t)n * T + tid] = expf(sm[tid] - mx) * inv;
  const float* xn = x + (size_t)q * T * D;
  for (int d = tid; d < D; d += 256) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += expf(sm[t] - mx) * inv * xn[(size_t)t * D + d];
    context[(size_t)n * D + d] = acc;
  }
}

extern "C" int tpgsr_aster_attention(const float* xproj, const float* sproj, const float* wv, const float* bv, const float* x, int N, int T,
                                     int A, int D, float* alpha, float* context, void* stream) {
  TPGSR_CHECK_ARG(xproj && sproj && wv && bv && x && alpha && context && N > 0 && T > 0 && T <= 256 && A > 0 && D > 0,
                  "tpgsr_aster_attention: bad arguments (T must be <= 256)");
  hipLaunchKernelGGL(aster_attention_kernel, dim3(N), dim3(256), T * sizeof(float), (hipStream_t)stream, xproj, sproj, wv, bv, x, 1, T, A,
                     D, alpha, context);
  TPGSR_LAUNCH_CHECK("tpgsr_aster_attention");
}

extern "C" int tpgsr_aster_attention_rows(const float* xproj, const float* sproj, const float* wv, const float* bv, const float* x, int R,
                                          int rows_per_seq, int T, int A, int D, float* alpha, float* context, void* stream) {
  TPGSR_CHECK_ARG(xproj && sproj && wv && bv && x && alpha && context, "tpgsr_aster_attention_rows: null pointer");
  TPGSR_CHECK_ARG(R > 0 && rows_per_seq > 0 && R % rows_per_seq == 0,
                  "tpgsr_aster_attention_rows: R must be a positive multiple of rows_per_seq >= 1 (got R %d, rows_per_seq %d)", R, rows_per_seq);
  TPGSR_CHECK_ARG(T > 0 && T <= 256 && A > 0 && D > 0, "tpgsr_aster_attention_rows: 1 <= T <= 256, A >= 1, D >= 1 (got T %d, A %d, D %d)", T,
                  A, D);
  hipLaunchKernelGGL(aster_attention_kernel, dim3(R), dim3(256), T * sizeof(float), (hipStream_t)stream, xproj, sproj, wv, bv, x, rows_per_seq,
                     T, A, D, alpha, context);
  TPGSR_LAUNCH_CHECK("tpgsr_aster_attention_rows");
}

// out[n] = [ emb[ids[n]] (E floats) | ctx[n] (D floats) ]
__global__ __launch_bounds__(256) void embed_concat_kernel(const int* __restrict__ ids, const float* __restrict__ emb, int V, int E,
                                                           const float* __restrict__ ctx, int D, int N, float* __restrict__ out) {
  const long long total = (long long)N * (E + D);
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i / (E + D)), j = (int)(i - (long long)n * (E + D));
  if (j < E) {
    int id = ids[n];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    out[i] = emb[(size_t)id * E + j];
  } else {
    out[i] = ctx[(size_t)n * D + (j - E)];
  }
}

extern "C" int tpgsr_embed_concat(const int* ids, const float* emb, int V, int E, const float* ctx, int D, int N, float* out, void* stream) {
  TPGSR_CHECK_ARG(ids && emb && ctx && out && V > 0 && E > 0 && D > 0 && N > 0, "tpgsr_embed_concat: bad arguments");
  hipLaunchKernelGGL(embed_concat_kernel, dim3(cdiv((long long)N * (E + D), 256)), dim3(256), 0, (hipStream_t)stream, ids, emb, V, E, ctx, D,
                     N, out);
  TPGSR_LAUNCH_CHECK("tpgsr_embed_concat");
}

// nn.GRU cell gate math (gate order r, z, n): h' = (1 - z) n + z h,  r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n)
__global__ __launch_bounds__(256) void gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                                                       int N, int Hd, float* __restrict__ hnew) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * Hd) return;
  const int n = (int)(i / Hd), j = (int)(i - (long long)n * Hd);
  const float* a = gi + (size_t)n * 3 * Hd;
  const float* b = gh + (size_t)n * 3 * Hd;
  const float r = sigmoid_f(a[j] + b[j]);
  const float z = sigmoid_f(a[Hd + j] + b[Hd + j]);
  const float nn_ = tanh_f(a[2 * Hd + j] + r * b[2 * Hd + j]);
  hnew[i] = (1.f - z) * nn_ + z * h[i];
}

extern "C" int tpgsr_gru_cell(const float* gi, const float* gh, const float* h, int N, int Hd, float* hnew, void* stream) {
  TPGSR_CHECK_ARG(gi && gh && h && hnew && N > 0 && Hd > 0, "tpgsr_gru_cell: bad arguments");
  hipLaunchKernelGGL(gru_cell_kernel, dim3(cdiv((long long)N * Hd, 256)), dim3(256), 0, (hipStream_t)stream, gi, gh, h, N, Hd, hnew);
  TPGSR_LAUNCH_CHECK("tpgsr_gru_cell");
}

// ids[n] = argmax_c logits[n][c] (first maximum, as torch.max), score[n] = softmax(logits[n])[ids[n]]; one wave per row;
// written at ids_out[n * ld + col] / score_out[n * ld + col] so a decode loop fills its (N, max_len) result in place
// A row without a finite maximum (all -inf, or all NaN) never satisfies `v > best`: its id stays INT_MAX and its score is NaN; the decode
// loop's next embed_concat clamps that id to V - 1 (tests/test_metric_decode_ops_gpu.py::test_softmax_max_row_without_a_maximum).
__global__ __launch_bounds__(64) void softmax_max_kernel(const float* __restrict__ logits, int C, int* __restrict__ ids, float* __restrict__ score,
                                                         int ld, int col, int* __restrict__ ids_next) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* p = logits + (size_t)n * C;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = p[c];
    if (v > best) {
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  float den = 0.f;
  for (int c = lane; c < C; c += 64) den += expf(p[c] - best);
  den = wave_sum(den);
  if (lane == 0) {
    ids[(size_t)n * ld + col] = bi;
    score[(size_t)n * ld + col] = 1.f / den;
    if (ids_next) ids_next[n] = bi;
  }
}

extern "C" int tpgsr_softmax_max(const float* logits, int N, int C, int* ids, float* score, int ld, int col, int* ids_next, void* stream) {
  TPGSR_CHECK_ARG(logits && ids && score && N > 0 && C > 0 && ld > col && col >= 0, "tpgsr_softmax_max: bad arguments");
  hipLaunchKernelGGL(softmax_max_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, logits, C, ids, score, ld, col, ids_next);
  TPGSR_LAUNCH_CHECK("tpgsr_softmax_max");
}

// ------------------------------------------------------------------------------------------------------
// Beam-search decode (AttentionRecognitionHead.beam_search, attention_recognition_head.py:68-184).  N images, B beams, C classes,
// row r = n * B + b.  One decoder step on all R = N B rows gives logits [R][C]; tpgsr_beam_step turns them into the step's B survivors
// per image, tpgsr_gather_rows reorders the decoder state by their predecessors, and after the last step tpgsr_beam_backtrack walks
// the stored histories once.  Nothing here is read back by the host.
//
// ORDER of every selection (torch.topk leaves equal values unordered): higher value first, then LOWER index (flat candidate index
// b * C + c, or slot index); a NaN counts as -inf; -inf candidates are taken, in index order, once the finite ones run out.
// ------------------------------------------------------------------------------------------------------
#define BEAM_MAX_B 8
#define BEAM_MAX_CAND 512                       // B * C: 8 candidates per lane, in registers
#define BEAM_PER_LANE (BEAM_MAX_CAND / 64)
#define BEAM_NONE 0x7fffffff

__device__ __forceinline__ float beam_key(float v) { return v != v ? -INFINITY : v; }      // NaN counts as -inf
// (value, index) of the better of two candidates under the order above; BEAM_NONE marks "no candidate"
__device__ __forceinline__ void beam_better(float& v, int& i, float ov, int oi) {
  if (oi != BEAM_NONE && (i == BEAM_NONE || ov > v || (ov == v && oi < i))) {
    v = ov;
    i = oi;
  }
}

// one wave per image: cand[b][c] = seq[n B + b] + log_softmax(logits[n B + b])[c]; the B best of the B C candidates, j-th best with
// flat index f -> row n B + j: symbol f % C, predecessor n B + f / C, its score; seq = the score, or -inf where the symbol is eos.
// f is always a real candidate index (< B C), so symbols lie in [0, C) and predecessors in [n B, n B + B) whatever the values are.
__global__ __launch_bounds__(64) void beam_step_kernel(const float* __restrict__ logits, float* __restrict__ seq, int B, int C, int eos,
                                                       float* __restrict__ score_t, int* __restrict__ sym_t, int* __restrict__ pred_t) {
  __shared__ float row_mx[BEAM_MAX_B], row_off[BEAM_MAX_B];      // per beam: max logit; running score - log sum exp
  const int n = blockIdx.x, lane = threadIdx.x, BC = B * C;
  const float* p = logits + (size_t)n * BC;
  for (int b = 0; b < B; ++b) {
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, p[b * C + c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float den = 0.f;
    for (int c = lane; c < C; c += 64) den += expf(p[b * C + c] - mx);
    den = wave_sum(den);
    if (lane == 0) {
      row_mx[b] = mx;
      row_off[b] = logf(den);
    }
  }
  __syncthreads();
  float v[BEAM_PER_LANE];
  unsigned taken = 0;                                             // bit k: candidate lane + 64 k is not (or no longer) available
#pragma unroll
  for (int k = 0; k < BEAM_PER_LANE; ++k) {
    const int f = lane + 64 * k;
    v[k] = -INFINITY;
    if (f < BC) {
      const int b = f / C;
      v[k] = beam_key(seq[n * B + b] + ((p[f] - row_mx[b]) - row_off[b]));      // as F.log_softmax: (x - max) - log(sum)
    } else {
      taken |= 1u << k;
    }
  }
  __syncthreads();                                               // every lane has read seq before lane 0 overwrites it
  for (int j = 0; j < B; ++j) {
    float best = -INFINITY;
    int bi = BEAM_NONE;
#pragma unroll
    for (int k = 0; k < BEAM_PER_LANE; ++k)
      if (!((taken >> k) & 1u)) beam_better(best, bi, v[k], lane + 64 * k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      beam_better(best, bi, ov, oi);
    }
    // B C >= B candidates and one is taken per round: bi is a real index here; the clamp keeps the guarantee unconditional
    bi = bi < 0 ? 0 : (bi >= BC ? BC - 1 : bi);
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    if (lane == 0) {
      const int r = n * B + j, sym = bi % C;
      score_t[r] = best;
      sym_t[r] = sym;
      pred_t[r] = n * B + bi / C;
      seq[r] = sym == eos ? -INFINITY : best;
    }
  }
}

extern "C" int tpgsr_beam_step(const float* logits, float* seq, int N, int B, int C, int eos, float* score_t, int* sym_t, int* pred_t,
                               void* stream) {
  TPGSR_CHECK_ARG(logits && seq && score_t && sym_t && pred_t, "tpgsr_beam_step: null pointer");
  TPGSR_CHECK_ARG(N > 0 && (long long)N * BEAM_MAX_CAND <= 0x7fffffffLL, "tpgsr_beam_step: N must be in 1 .. 2^31 / %d (got %d)", BEAM_MAX_CAND, N);
  TPGSR_CHECK_ARG(B >= 1 && B <= BEAM_MAX_B, "tpgsr_beam_step: beam width B must be in 1 .. %d (got %d)", BEAM_MAX_B, B);
  TPGSR_CHECK_ARG(C >= 1 && (long long)B * C <= BEAM_MAX_CAND, "tpgsr_beam_step: C >= 1 and B * C <= %d candidates per image (got B %d, C %d)",
                  BEAM_MAX_CAND, B, C);
  hipLaunchKernelGGL(beam_step_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, logits, seq, B, C, eos, score_t, sym_t, pred_t);
  TPGSR_LAUNCH_CHECK("tpgsr_beam_step");
}

// dst[r] = src[idx[r]], rows of W floats (the decoder state after a beam step); an index outside [0, R) is clamped, never followed.
// 16-byte pieces where W and both pointers allow it.
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(const V* __restrict__ src, const int* __restrict__ idx, int R, int Wv,
                                                          V* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)R * Wv) return;
  const int r = (int)(i / Wv), j = (int)(i - (long long)r * Wv);
  int s = idx[r];
  s = s < 0 ? 0 : (s >= R ? R - 1 : s);
  dst[i] = src[(size_t)s * Wv + j];
}

extern "C" int tpgsr_gather_rows(const float* src, const int* idx, int R, int W, float* dst, void* stream) {
  TPGSR_CHECK_ARG(src && idx && dst, "tpgsr_gather_rows: null pointer");
  TPGSR_CHECK_ARG(src != dst, "tpgsr_gather_rows: src and dst must be different buffers");
  TPGSR_CHECK_ARG(R > 0 && W > 0, "tpgsr_gather_rows: R and W must be at least 1 (got R %d, W %d)", R, W);
  const bool vec = W % 4 == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  const int Wv = vec ? W / 4 : W;
  const long long total = (long long)R * Wv;
  TPGSR_CHECK_ARG(total <= 0x7fffffffLL * 256, "tpgsr_gather_rows: R * W = %lld elements exceed the grid limit", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(gather_rows_kernel<floatx4>, grid, dim3(256), 0, (hipStream_t)stream, (const floatx4*)src, idx, R, Wv, (floatx4*)dst);
  else
    hipLaunchKernelGGL(gather_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src, idx, R, Wv, dst);
  TPGSR_LAUNCH_CHECK("tpgsr_gather_rows");
}

// The backtrack of one image, one wave, slot k in lane k (k < B).  Histories are [L][R].  The slots start as the last step's rows in
// descending score order; walking t = L-1 .. 0 every slot reads its symbol through its back pointer and moves the pointer to the
// predecessor, then every row of the image that emitted eos at t (descending row order; k-th such row of the whole walk) takes over
// slot B - 1 - (k mod B): back pointer, symbol, score and length t + 1.  The best slot after the walk is the result.
// Which slot is best is known only after the walk and the symbols of B slots over L steps have no home (L is unbounded), so the walk
// runs twice: once for scores and lengths, once more with the best slot's lane writing its symbols.  A back pointer read from the
// history is clamped into the image's rows before it is followed.
template <bool EMIT>
__device__ __forceinline__ void beam_walk(const float* __restrict__ score_hist, const int* __restrict__ sym_hist,
                                          const int* __restrict__ pred_hist, int n, int B, int L, int R, int eos, int lane, int ptr0,
                                          float& score, int& len, int emit_lane, int* __restrict__ ids_row) {
  const int lo = n * B, hi = n * B + B - 1;
  int ptr = ptr0, found = 0;
  for (int t = L - 1; t >= 0; --t) {
    const int* sym_t = sym_hist + (size_t)t * R;
    const int* pred_t = pred_hist + (size_t)t * R;
    int sym = sym_t[ptr];
    int nxt = pred_t[ptr];
    const int own = lane < B ? lo + lane : lo;                   // lane b looks at row n B + b of this step
    const unsigned long long ended = __ballot(lane < B && sym_t[own] == eos);
    const int own_pred = pred_t[own];
    const float own_score = score_hist[(size_t)t * R + own];
    for (int b = B - 1; b >= 0; --b) {
      if (!((ended >> b) & 1ull)) continue;                      // (wave-uniform)
      const int slot = B - 1 - (found % B);
      ++found;
      const int rp = __shfl(own_pred, b);
      const float rs = __shfl(own_score, b);
      if (lane == slot) {
        nxt = rp;
        sym = eos;
        score = rs;
        len = t + 1;
      }
    }
    ptr = nxt < lo ? lo : (nxt > hi ? hi : nxt);
    if (EMIT && lane == emit_lane) ids_row[t] = sym;
  }
}

__global__ __launch_bounds__(64) void beam_backtrack_kernel(const float* __restrict__ score_hist, const int* __restrict__ sym_hist,
                                                            const int* __restrict__ pred_hist, int N, int B, int L, int eos,
                                                            int* __restrict__ ids_out, float* __restrict__ best_score,
                                                            int* __restrict__ best_len) {
  __shared__ float slot_score[BEAM_MAX_B];
  __shared__ int slot_ptr[BEAM_MAX_B];
  const int n = blockIdx.x, lane = threadIdx.x, R = N * B;
  const int me = lane < B ? lane : 0;
  // the last step's rows in descending score order: rank = how many rows come before this one
  const float mine = score_hist[(size_t)(L - 1) * R + n * B + me];
  int rank = 0;
  for (int i = 0; i < B; ++i) {
    const float o = beam_key(__shfl(mine, i));
    rank += (o > beam_key(mine) || (o == beam_key(mine) && i < me)) ? 1 : 0;
  }
  if (lane < B) {
    slot_score[rank] = mine;
    slot_ptr[rank] = n * B + lane;
  }
  __syncthreads();
  const float score0 = slot_score[me];
  const int ptr0 = slot_ptr[me];
  float score = score0;
  int len = L;
  beam_walk<false>(score_hist, sym_hist, pred_hist, n, B, L, R, eos, lane, ptr0, score, len, 0, nullptr);
  // the best slot: highest score, then lowest slot index
  float bs = lane < B ? beam_key(score) : -INFINITY;
  int bk = lane < B ? lane : BEAM_NONE;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bs, o);
    const int ok = __shfl_xor(bk, o);
    beam_better(bs, bk, ov, ok);
  }
  bk = bk < 0 ? 0 : (bk >= B ? B - 1 : bk);
  if (lane == bk) {
    best_score[n] = score;
    best_len[n] = len;
  }
  score = score0;
  len = L;
  beam_walk<true>(score_hist, sym_hist, pred_hist, n, B, L, R, eos, lane, ptr0, score, len, bk, ids_out + (size_t)n * L);
}

extern "C" int tpgsr_beam_backtrack(const float* score_hist, const int* sym_hist, const int* pred_hist, int N, int B, int L, int eos,
                                    int* ids_out, float* best_score, int* best_len, void* stream) {
  TPGSR_CHECK_ARG(score_hist && sym_hist && pred_hist && ids_out && best_score && best_len, "tpgsr_beam_backtrack: null pointer");
  TPGSR_CHECK_ARG(B >= 1 && B <= BEAM_MAX_B, "tpgsr_beam_backtrack: beam width B must be in 1 .. %d (got %d)", BEAM_MAX_B, B);
  TPGSR_CHECK_ARG(N > 0 && L >= 1, "tpgsr_beam_backtrack: N and L must be at least 1 (got N %d, L %d)", N, L);
  TPGSR_CHECK_ARG((long long)N * B <= 0x7fffffffLL && (long long)N * L <= 0x7fffffffLL,
                  "tpgsr_beam_backtrack: N * B and N * L must stay below 2^31 (got N %d, B %d, L %d)", N, B, L);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, score_hist, sym_hist, pred_hist, N, B, L, eos, ids_out,
                     best_score, best_len);
  TPGSR_LAUNCH_CHECK("tpgsr_beam_backtrack");
}
