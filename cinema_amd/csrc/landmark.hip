// Landmark localisation (reference cinema/segmentation/landmark/train.py and cinema/regression/landmark/train.py): the heatmap loss of the detection
// fine-tuning step (sigmoid soft Dice + BCE-with-logits against soft Gaussian labels), sliding-window aggregation in sigmoid space, the heatmap metrics
// (soft-argmax coordinates, per-map Dice) and the Wing loss of the coordinate-regression head.
// Every reduction is formed in a fixed order (wave butterflies, per-block partial slabs, a fixed-order finish): no float atomics, so the same inputs
// give bitwise-equal outputs.
#include "common.cuh"
#include "../../include/cinema_hip.h"

namespace {

constexpr int LM_MAXC = 16;
constexpr int LM_MAXG = CINEMA_LANDMARK_MAX_BLOCKS;  // blocks per sample of the loss forward = partial rows per sample in the slab
static_assert(LM_MAXG <= 64, "the finish kernel sums the partial rows of one (sample, channel) across the 64 lanes of a wave");

// sigmoid from e = exp(-|x|) (never overflows): x >= 0: 1 / (1 + e), else e / (1 + e); v_rcp_f32 (1 ulp) instead of the IEEE division sequence
__device__ __forceinline__ float sigmoid_e(float x, float e) {
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return x >= 0.f ? r : e * r;
}
__device__ __forceinline__ float sigmoid_f(float x) { return sigmoid_e(x, __expf(-fabsf(x))); }

// ---- heatmap loss: per (sample, channel) I = sum sigma(x) t, P = sum sigma(x), G = sum t and the BCE sum, one slab row per block -------------------
// logits channels-last rows [b * vox][c], labels channels-first [b][c][vox]; slab [b][gridDim.x][3c + 1]: (I, P, G) per channel, then the BCE sum.
// NC: compile-time bound of c (c <= NC), so that the per-channel accumulators stay in registers (fully unrolled loops, no dynamic indexing)
template <int NC>
__global__ __launch_bounds__(256) void landmark_loss_fwd_kernel(const float* logits, const float* labels, int vox, int c, float* slab) {
  __shared__ float red[4][NC * 3 + 1];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float li[NC], lp[NC], lt[NC], bce = 0.f;
#pragma unroll
  for (int j = 0; j < NC; j++) { li[j] = 0.f; lp[j] = 0.f; lt[j] = 0.f; }
  const float* lab = labels + (size_t)b * c * vox;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < vox; v += gridDim.x * 256) {
    const float* row = logits + ((size_t)b * vox + v) * c;
#pragma unroll
    for (int j = 0; j < NC; j++) {
      if (j < c) {
        const float x = row[j], t = lab[(size_t)j * vox + v];
        const float e = __expf(-fabsf(x));
        const float s = sigmoid_e(x, e);
        li[j] += s * t; lp[j] += s; lt[j] += t;
        bce += fmaxf(x, 0.f) - x * t + __logf(1.f + e);  // BCEWithLogitsLoss, stable for any |x| (log(1 + e) for e in (0, 1]: absolute error ~1e-7)
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; j++) {
    if (j < c) {
      const float a = wave_sum(li[j]), p = wave_sum(lp[j]), t = wave_sum(lt[j]);
      if (lane == 0) { red[wave][3 * j] = a; red[wave][3 * j + 1] = p; red[wave][3 * j + 2] = t; }
    }
  }
  bce = wave_sum(bce);
  if (lane == 0) red[wave][3 * c] = bce;
  __syncthreads();
  float* out = slab + ((size_t)b * gridDim.x + blockIdx.x) * (3 * c + 1);
  for (int i = threadIdx.x; i < 3 * c + 1; i += 256) out[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// Fixed-order tree sum of one value per thread over the block (256 threads); the result is returned to every thread.
__device__ __forceinline__ float block_sum_fixed(float v, float* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const float r = sh[0];
  __syncthreads();
  return r;
}

// out4 = {loss, bce, dice, 0}; coef[b][c] = (d dice / d I, d dice / d P).  monai DiceLoss defaults: smooth_nr = smooth_dr = 1e-5, mean over b * c.
// 1024 threads: one wave per (sample, channel), its lanes over the g <= 64 partial rows (fixed-order butterfly), then fixed-order block sums.
__global__ __launch_bounds__(1024) void landmark_loss_finish_kernel(const float* slab, int b, int c, int g, float inv_n, float* out4, float* coef) {
  __shared__ float sh[1024];
  const int w = 3 * c + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_bc = 1.f / (float)(b * c);
  float dice = 0.f, bce = 0.f;
  // the slab was written by other XCDs: every read is a memory round trip, so a wave issues the loads of FIN_ITEMS items before it sums any
  // (one serial round per item took 12 us for the 96 maps of batch 32)
  constexpr int FIN_ITEMS = 8;
  for (int i0 = wave; i0 < b * c; i0 += 16 * FIN_ITEMS) {
    float vi[FIN_ITEMS], vp[FIN_ITEMS], vg[FIN_ITEMS];
#pragma unroll
    for (int u = 0; u < FIN_ITEMS; u++) {
      const int i = i0 + 16 * u;
      const bool on = lane < g && i < b * c;
      const float* r = slab + (on ? ((size_t)(i / c) * g + lane) * w + 3 * (i % c) : 0);
      vi[u] = on ? r[0] : 0.f; vp[u] = on ? r[1] : 0.f; vg[u] = on ? r[2] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < FIN_ITEMS; u++) {
      const int i = i0 + 16 * u;
      const float I = wave_sum(vi[u]), P = wave_sum(vp[u]), G = wave_sum(vg[u]);
      const float den = G + P + 1e-5f, num = 2.f * I + 1e-5f;
      if (lane == 0 && i < b * c) {
        dice += 1.f - num / den;
        coef[2 * i] = -2.f / den * inv_bc;
        coef[2 * i + 1] = num / (den * den) * inv_bc;
      }
    }
  }
#pragma unroll 4
  for (int i = threadIdx.x; i < b * g; i += 1024) bce += slab[(size_t)i * w + 3 * c];
  sh[threadIdx.x] = dice;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  dice = sh[0] * inv_bc;
  __syncthreads();
  sh[threadIdx.x] = bce;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) { bce = sh[0] * inv_n; out4[0] = bce + dice; out4[1] = bce; out4[2] = dice; out4[3] = 0.f; }
}

// dlogits [b * vox][c] = up * ((sigma - t) / (b c vox) + sigma (1 - sigma) (coef_I t + coef_P))
template <int NC>
__global__ __launch_bounds__(256) void landmark_loss_bwd_kernel(const float* logits, const float* labels, int vox, int c, const float* coef, float inv_n,
                                                                const float* upstream, float* dlogits) {
  const int b = blockIdx.y;
  const float up = upstream ? upstream[0] : 1.f;
  float ci[NC], cp[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) { ci[j] = j < c ? coef[(b * c + j) * 2] : 0.f; cp[j] = j < c ? coef[(b * c + j) * 2 + 1] : 0.f; }
  const float* lab = labels + (size_t)b * c * vox;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < vox; v += gridDim.x * 256) {
    const size_t r = ((size_t)b * vox + v) * c;
#pragma unroll
    for (int j = 0; j < NC; j++) {
      if (j < c) {
        const float t = lab[(size_t)j * vox + v];
        const float s = sigmoid_f(logits[r + j]);
        dlogits[r + j] = up * ((s - t) * inv_n + s * (1.f - s) * (ci[j] * t + cp[j]));
      }
    }
  }
}

int loss_blocks(int vox) { const int g = (vox + 255) / 256; return g < LM_MAXG ? g : LM_MAXG; }

// ---- sliding-window aggregation in sigmoid space --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void landmark_window_accumulate_kernel(const float* logits, int c, int px, int py, int pz, int sx, int sy, int sz, int Y, int Z,
                                                                         float* prob_sum, float* count) {
  const int nvox = px * py * pz;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    const int z = v % pz, y = (v / pz) % py, x = v / (pz * py);
    const size_t o = ((size_t)(x + sx) * Y + (y + sy)) * Z + (z + sz);
    for (int j = 0; j < c; j++) prob_sum[o * c + j] += 1.f / (1.f + expf(-logits[(size_t)v * c + j]));
    count[o] += 1.f;
  }
}

// out[j * nvox + v] = log(p / (1 - p)), p = prob_sum[v][j] / count[v] (unclamped: p == 1 gives +inf, as the reference)
__global__ __launch_bounds__(256) void landmark_window_finish_kernel(const float* prob_sum, const float* count, int c, long long nvox, float* out) {
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nvox; v += (long long)gridDim.x * 256) {
    const float n = count[v];
    for (int j = 0; j < c; j++) {
      const float p = prob_sum[v * c + j] / n;
      out[(size_t)j * nvox + v] = logf(p / (1.f - p));
    }
  }
}

// ---- heatmap metrics: one workgroup per (sample, channel) map ---------------------------------------------------------------------------------------
// online soft-argmax state: running maximum m of beta * value, s = sum exp(beta v - m), sx / sy = the same sums weighted by the coordinates
struct SoftArg { float m, s, sx, sy; };

__device__ __forceinline__ void sa_add(SoftArg& a, float u, float x, float y) {
  if (u > a.m) {
    const float k = a.s > 0.f ? expf(a.m - u) : 0.f;
    a.s = a.s * k + 1.f; a.sx = a.sx * k + x; a.sy = a.sy * k + y; a.m = u;
  } else {
    const float e = expf(u - a.m);
    a.s += e; a.sx += e * x; a.sy += e * y;
  }
}
__device__ __forceinline__ SoftArg sa_merge(SoftArg a, SoftArg b) {
  if (b.s == 0.f) return a;
  if (a.s == 0.f) return b;
  const float m = fmaxf(a.m, b.m), ka = expf(a.m - m), kb = expf(b.m - m);
  return SoftArg{m, a.s * ka + b.s * kb, a.sx * ka + b.sx * kb, a.sy * ka + b.sy * kb};
}
__device__ __forceinline__ SoftArg sa_wave(SoftArg a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    SoftArg b{__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64), __shfl_xor(a.sx, o, 64), __shfl_xor(a.sy, o, 64)};
    a = (threadIdx.x & o) ? sa_merge(b, a) : sa_merge(a, b);  // the same operand order on both partners of a pair
  }
  return a;
}

// out [b][c][8] = {E[x], E[y] of softmax(beta * sigmoid(logits)), E[x], E[y] of softmax(beta * labels), I, P, G, 1 - (2I + 1e-5) / (G + P + 1e-5)}
// logits / labels channels-first [b][c][w * h], element (x, y) at x * h + y (torch.cartesian_prod(arange(w), arange(h)) order)
__global__ __launch_bounds__(256) void heatmap_metrics_kernel(const float* logits, const float* labels, int w, int h, float beta, float* out) {
  __shared__ float sh[4][11];
  const int j = blockIdx.x, c = gridDim.x, b = blockIdx.y, n = w * h;
  const float* lg = logits + ((size_t)b * c + j) * n;
  const float* lb = labels + ((size_t)b * c + j) * n;
  SoftArg sp{-INFINITY, 0.f, 0.f, 0.f}, st{-INFINITY, 0.f, 0.f, 0.f};
  float I = 0.f, P = 0.f, G = 0.f;
  for (int v = threadIdx.x; v < n; v += 256) {
    const float x = (float)(v / h), y = (float)(v % h);
    const float p = 1.f / (1.f + expf(-lg[v])), t = lb[v];
    sa_add(sp, beta * p, x, y);
    sa_add(st, beta * t, x, y);
    I += p * t; P += p; G += t;
  }
  sp = sa_wave(sp); st = sa_wave(st);
  I = wave_sum(I); P = wave_sum(P); G = wave_sum(G);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    float* r = sh[wave];
    r[0] = sp.m; r[1] = sp.s; r[2] = sp.sx; r[3] = sp.sy; r[4] = st.m; r[5] = st.s; r[6] = st.sx; r[7] = st.sy; r[8] = I; r[9] = P; r[10] = G;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    SoftArg ap{sh[0][0], sh[0][1], sh[0][2], sh[0][3]}, at{sh[0][4], sh[0][5], sh[0][6], sh[0][7]};
    float sI = sh[0][8], sP = sh[0][9], sG = sh[0][10];
    for (int k = 1; k < 4; k++) {
      ap = sa_merge(ap, SoftArg{sh[k][0], sh[k][1], sh[k][2], sh[k][3]});
      at = sa_merge(at, SoftArg{sh[k][4], sh[k][5], sh[k][6], sh[k][7]});
      sI += sh[k][8]; sP += sh[k][9]; sG += sh[k][10];
    }
    float* o = out + ((size_t)b * c + j) * 8;
    o[0] = ap.sx / ap.s; o[1] = ap.sy / ap.s; o[2] = at.sx / at.s; o[3] = at.sy / at.s;
    o[4] = sI; o[5] = sP; o[6] = sG; o[7] = 1.f - (2.f * sI + 1e-5f) / (sG + sP + 1e-5f);
  }
}

// ---- Wing loss of the coordinate head -------------------------------------------------------------------------------------------------------------
// relative distances (get_relative_distances): rel = coords @ M, M symmetric: point 1 minus the midpoint of points 2 and 3, and so on
__constant__ float REL_M[6][6] = {{1.f, 0.f, -.5f, 0.f, -.5f, 0.f}, {0.f, 1.f, 0.f, -.5f, 0.f, -.5f}, {-.5f, 0.f, 1.f, 0.f, -.5f, 0.f},
                                  {0.f, -.5f, 0.f, 1.f, 0.f, -.5f}, {-.5f, 0.f, -.5f, 0.f, 1.f, 0.f}, {0.f, -.5f, 0.f, -.5f, 0.f, 1.f}};

__device__ __forceinline__ float wing_f(float e, float w, float eps, float C) { return e < w ? w * logf(1.f + e / eps) : e - C; }
// d wing(|d|) / d d: sign(d) * wing'(|d|); sign(0) = 0 (the gradient torch.abs gives at 0)
__device__ __forceinline__ float wing_g(float d, float w, float eps) {
  const float e = fabsf(d);
  const float g = e < w ? w / (eps + e) : 1.f;
  return d > 0.f ? g : (d < 0.f ? -g : 0.f);
}

__global__ __launch_bounds__(256) void head_wing_kernel(const float* pred, const float* label, const float* scales, int b, int n, float w, float eps, int rel,
                                                        float* out5, float* dpred) {
  __shared__ float sh[256];
  const float C = w - w * logf(1.f + w / eps);
  const float inv = 1.f / (float)(b * n);
  float lw = 0.f, rw = 0.f, lm = 0.f, rm = 0.f;
  for (int i = threadIdx.x; i < b; i += 256) {
    float P[6], T[6], S[6], dP[6];
    for (int k = 0; k < n; k++) {
      const size_t o = (size_t)i * n + k;
      const float sc = scales ? scales[o] : 1.f;
      const float p = pred[o] * sc, t = label[o] * sc;
      const float d = p - t;
      lw += wing_f(fabsf(d), w, eps, C); lm += fabsf(d);
      if (rel) { P[k] = p; T[k] = t; S[k] = sc; dP[k] = wing_g(d, w, eps) * inv; }  // (rel: n == 6)
      else dpred[o] = wing_g(d, w, eps) * inv * sc;
    }
    if (!rel) continue;
    float gr[6];
    for (int m = 0; m < 6; m++) {
      float rp = 0.f, rt = 0.f;
      for (int k = 0; k < 6; k++) { rp += P[k] * REL_M[k][m]; rt += T[k] * REL_M[k][m]; }
      const float d = rp - rt;
      rw += wing_f(fabsf(d), w, eps, C); rm += fabsf(d);
      gr[m] = wing_g(d, w, eps) * inv;
    }
    for (int k = 0; k < 6; k++) {
      float g = dP[k];
      for (int m = 0; m < 6; m++) g += REL_M[k][m] * gr[m];
      dpred[(size_t)i * 6 + k] = g * S[k];
    }
  }
  lw = block_sum_fixed(lw, sh); rw = block_sum_fixed(rw, sh); lm = block_sum_fixed(lm, sh); rm = block_sum_fixed(rm, sh);
  if (threadIdx.x == 0) { out5[0] = (lw + rw) * inv; out5[1] = lw * inv; out5[2] = rw * inv; out5[3] = lm * inv; out5[4] = rm * inv; }
}

}  // namespace

CINEMA_API int cinema_landmark_loss_fwd(const float* logits, const float* labels, int b, int vox, int c, float* slab, float* out4, float* coef, void* stream) {
  if (!logits || !labels || !slab || !out4 || !coef || b <= 0 || vox <= 0 || c < 1) return CINEMA_ERR_BAD_ARG;
  if (c > LM_MAXC || (long long)b * vox * c >= (1LL << 40)) return CINEMA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int g = loss_blocks(vox);
  if (c <= 4)
    CINEMA_LAUNCH(landmark_loss_fwd_kernel<4>, dim3(g, b), dim3(256), 0, st, logits, labels, vox, c, slab);
  else
    CINEMA_LAUNCH(landmark_loss_fwd_kernel<LM_MAXC>, dim3(g, b), dim3(256), 0, st, logits, labels, vox, c, slab);
  CINEMA_LAUNCH(landmark_loss_finish_kernel, dim3(1), dim3(1024), 0, st, (const float*)slab, b, c, g, (float)(1.0 / ((double)b * c * vox)), out4, coef);
  return launch_status();
}

CINEMA_API int cinema_landmark_loss_bwd(const float* logits, const float* labels, int b, int vox, int c, const float* coef, const float* upstream,
                                        float* dlogits, void* stream) {
  if (!logits || !labels || !coef || !dlogits || b <= 0 || vox <= 0 || c < 1) return CINEMA_ERR_BAD_ARG;
  if (c > LM_MAXC) return CINEMA_ERR_UNSUPPORTED;
  int gx = (vox + 255) / 256;
  if (gx > 2048) gx = 2048;
  const float inv_n = (float)(1.0 / ((double)b * c * vox));
  if (c <= 4)
    CINEMA_LAUNCH(landmark_loss_bwd_kernel<4>, dim3(gx, b), dim3(256), 0, (hipStream_t)stream, logits, labels, vox, c, coef, inv_n, upstream, dlogits);
  else
    CINEMA_LAUNCH(landmark_loss_bwd_kernel<LM_MAXC>, dim3(gx, b), dim3(256), 0, (hipStream_t)stream, logits, labels, vox, c, coef, inv_n, upstream, dlogits);
  return launch_status();
}

CINEMA_API int cinema_landmark_window_accumulate(const float* window_logits, int c, int px, int py, int pz, int sx, int sy, int sz, int X, int Y, int Z,
                                                 float* prob_sum, float* count, void* stream) {
  if (!window_logits || !prob_sum || !count || c < 1 || px <= 0 || py <= 0 || pz <= 0 || sx < 0 || sy < 0 || sz < 0 || sx + px > X || sy + py > Y || sz + pz > Z)
    return CINEMA_ERR_BAD_ARG;
  int gx = (px * py * pz + 255) / 256;
  if (gx > 4096) gx = 4096;
  CINEMA_LAUNCH(landmark_window_accumulate_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, window_logits, c, px, py, pz, sx, sy, sz, Y, Z, prob_sum, count);
  return launch_status();
}

CINEMA_API int cinema_landmark_window_finish(const float* prob_sum, const float* count, int c, long long n_voxels, float* logits_out, void* stream) {
  if (!prob_sum || !count || !logits_out || c < 1 || n_voxels <= 0) return CINEMA_ERR_BAD_ARG;
  long long gx = (n_voxels + 255) / 256;
  if (gx > 4096) gx = 4096;
  CINEMA_LAUNCH(landmark_window_finish_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, prob_sum, count, c, n_voxels, logits_out);
  return launch_status();
}

CINEMA_API int cinema_heatmap_metrics(const float* logits, const float* labels, int b, int c, int w, int h, float beta, float* out, void* stream) {
  if (!logits || !labels || !out || b <= 0 || c <= 0 || w <= 0 || h <= 0 || b > 65535) return CINEMA_ERR_BAD_ARG;
  if ((long long)w * h >= (1LL << 31)) return CINEMA_ERR_UNSUPPORTED;
  CINEMA_LAUNCH(heatmap_metrics_kernel, dim3(c, b), dim3(256), 0, (hipStream_t)stream, logits, labels, w, h, beta, out);
  return launch_status();
}

CINEMA_API int cinema_head_wing(const float* pred, const float* label, const float* scales, int b, int n, float w, float epsilon, int rel, float* out5,
                                float* dpred, void* stream) {
  if (!pred || !label || !out5 || !dpred || b <= 0 || n <= 0 || !(w > 0.f) || !(epsilon > 0.f)) return CINEMA_ERR_BAD_ARG;
  if (rel && n != 6) return CINEMA_ERR_BAD_ARG;
  CINEMA_LAUNCH(head_wing_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, label, scales, b, n, w, epsilon, rel, out5, dpred);
  return launch_status();
}
