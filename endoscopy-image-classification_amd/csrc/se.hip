// The squeeze-excite tail of an SE-ResNet bottleneck (code/models/se.py:32-58), fused with the block's last
// BatchNorm, the residual add and the ReLU:
//
//   y = conv3's output [N, HW, C] (NHWC, fp32 or bf16), o = gamma (y - mean) rstd + beta = bn3(y), never written
//   a = pool_hw(o) = gamma (pool_hw(y) - mean) rstd + beta          (the pool of an affine map: no pass over o)
//   h = relu(a W_down^T) [N, R],  s = sigmoid(h W_up^T) [N, C]
//   out = relu(s o + res)                                            (one read of y and res, one write)
//
//  es_se_bn_stats          mean / rstd (+ running buffers) from channel sums (train), or from the running
//                          statistics (eval), where conv3's epilogue partials are not available
//  es_se_squeeze_ex        y -> ybar [N, C], a [N, C]              one read of y
//  es_se_gate_fwd          a, W_down, W_up -> h, s                 [N, C]-sized
//  es_se_bn_apply_ex       y, res, s -> out                        the BatchNorm apply pass with a gate
//  es_se_bn_bwd_sums_ex    y, out, dout -> P1 = sum_hw g, P2 = sum_hw g xhat  (g = dout [out > 0])
//  es_se_gate_bwd          P1, P2, ... -> dW_down, dW_up, da, dgamma, dbeta   [N, C]-sized
//  es_se_bn_bwd_dx_ex      y, out, dout, s, da, ... -> dy, gres    the BatchNorm backward's dx pass with a gate
//
// Per direction that is BatchNorm's own two passes over the maps (forward: statistics from conv3's epilogue, so
// the squeeze is the one added read).  Every sum is taken in a fixed order (per-workgroup partials combined by
// a second launch, no float atomics): repeated launches give the same bits.  Every output element is written.
// Maps move as 16-byte vectors (8 bf16 / 4 fp32 per lane), so C % 16 == 0 and 16-byte aligned pointers.
#include <numeric>

#include "common.h"

namespace {

constexpr int SE_MAPS_BF16 = 1;
constexpr int SE_MAX_C = 2048, SE_MAX_R = 128;

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int VEC>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&o)[VEC]) {
#pragma unroll
  for (int h = 0; h < VEC / 4; ++h) {
    const f32x4 t = *(const f32x4*)(p + 4 * h);
    o[4 * h] = t[0]; o[4 * h + 1] = t[1]; o[4 * h + 2] = t[2]; o[4 * h + 3] = t[3];
  }
}
template <int VEC>
__device__ __forceinline__ void ldv(const bf16* __restrict__ p, float (&o)[VEC]) {
  static_assert(VEC == 8, "bf16 maps move 8 elements per lane");
  const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (float)t[j];
}
template <int VEC>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&v)[VEC]) {
#pragma unroll
  for (int h = 0; h < VEC / 4; ++h) *(f32x4*)(p + 4 * h) = f32x4{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
}
template <int VEC>
__device__ __forceinline__ void stv(bf16* __restrict__ p, const float (&v)[VEC]) {
  static_assert(VEC == 8, "bf16 maps move 8 elements per lane");
  bf16x8 t;
#pragma unroll
  for (int j = 0; j < 8; ++j) t[j] = (bf16)v[j];
  *(bf16x8*)p = t;
}
template <typename T>
struct MapVec {
  static constexpr int V = sizeof(T) == 2 ? 8 : 4;  // one 16-byte access
};

// ---- per-(image, channel) sums over HW: the squeeze (SUMS = false: sum y) and the backward's sums pass
// (SUMS = true: sum g, sum g xhat).  Workgroup (split, image, channel chunk): a thread owns VEC channels and
// walks every rp-th row of the split's rows (chan_partial_kernel's scheme, conv.hip), then the row lanes are
// combined through LDS in a fixed order.  partial[(n S + split)][c] (SUMS: [2][c]).
template <typename T, int VEC, bool SUMS>
__global__ __launch_bounds__(256) void se_partial_kernel(const T* __restrict__ y, const T* __restrict__ out,
                                                         const T* __restrict__ dout, int HW, int C, int per, int S,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ partial) {
  __shared__ float red[256 * VEC];
  __shared__ float red2[SUMS ? 256 * VEC : 1];
  const int CV = C / VEC;
  const int cpp = CV < 256 ? CV : 256;  // vector columns of this workgroup
  const int rp = 256 / cpp;             // row lanes
  const int t = threadIdx.x, cc = t % cpp, rl = t / cpp;
  const int sp = blockIdx.x, n = blockIdx.y, c0 = blockIdx.z * cpp;
  const int cv = c0 + cc, c = cv * VEC;
  const int r0 = sp * per, r1 = min(r0 + per, HW);
  const long base = (long)n * HW * C;
  float s[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = s2[j] = 0.f;
  if (rl < rp && cv < CV) {
    float mu[VEC], rs[VEC];
    if constexpr (SUMS) {
      ldv<VEC>(mean + c, mu);
      ldv<VEC>(rstd + c, rs);
    }
    auto acc = [&](int r) {
      const long o = base + (long)r * C + c;
      float a[VEC];
      ldv<VEC>(y + o, a);
      if constexpr (!SUMS) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += a[j];
      } else {
        float gd[VEC], oo[VEC];
        ldv<VEC>(dout + o, gd);
        ldv<VEC>(out + o, oo);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float gg = oo[j] > 0.f ? gd[j] : 0.f;
          s[j] += gg;
          s2[j] = fmaf(gg, (a[j] - mu[j]) * rs[j], s2[j]);
        }
      }
    };
    int r = r0 + rl;
    for (; r + 3 * rp < r1; r += 4 * rp) {
      acc(r);
      acc(r + rp);
      acc(r + 2 * rp);
      acc(r + 3 * rp);
    }
    for (; r < r1; r += rp) acc(r);
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    red[t * VEC + j] = s[j];
    if constexpr (SUMS) red2[t * VEC + j] = s2[j];
  }
  __syncthreads();
  const int width = SUMS ? 2 * C : C;
  float* dst = partial + ((long)n * S + sp) * width;
  for (int q = t; q < cpp * VEC && c0 * VEC + q < C; q += 256) {
    const int col = q / VEC, j = q % VEC;
    float a = 0.f, b = 0.f;
    for (int l = 0; l < rp; ++l) {
      a += red[(l * cpp + col) * VEC + j];
      if constexpr (SUMS) b += red2[(l * cpp + col) * VEC + j];
    }
    dst[c0 * VEC + q] = a;
    if constexpr (SUMS) dst[C + c0 * VEC + q] = b;
  }
}

// the splits of one (image, channel) summed in order: ybar = sum / HW, a = bn3's affine map at ybar
__global__ __launch_bounds__(256) void se_squeeze_final_kernel(const float* __restrict__ partial, int N, int HW, int C,
                                                               int S, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ ybar,
                                                               float* __restrict__ a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * C) return;
  const int n = (int)(i / C), c = (int)(i - (long)n * C);
  const float* p = partial + (long)n * S * C + c;
  float sum = 0.f;
  for (int k = 0; k < S; k += 8) {  // 8 loads in flight, added in order (a split past S adds 0)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = k + u < S ? p[(long)(k + u) * C] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  const float yb = __fdiv_rn(sum, (float)HW);  // correctly rounded: exact where HW divides the sum
  ybar[i] = yb;
  a[i] = bn_affine(yb, mean[c], rstd[c], gamma[c], beta[c]);
}

__global__ __launch_bounds__(256) void se_sums_final_kernel(const float* __restrict__ partial, int N, int C, int S,
                                                            float* __restrict__ p1, float* __restrict__ p2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * C) return;
  const int n = (int)(i / C), c = (int)(i - (long)n * C);
  const float* p = partial + (long)n * S * 2 * C + c;
  float u = 0.f, v = 0.f;
  for (int k = 0; k < S; k += 8) {  // 16 loads in flight, added in order
    float a[8], b[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q] = k + q < S ? p[(long)(k + q) * 2 * C] : 0.f;
      b[q] = k + q < S ? p[(long)(k + q) * 2 * C + C] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      u += a[q];
      v += b[q];
    }
  }
  p1[i] = u;
  p2[i] = v;
}

// ---- the gate: [N, C]- and [N, R]-sized products, tiled so that a 64-image batch fills more than 64 workgroups
constexpr int SE_GN = 16;    // images per workgroup of se_gate_s_kernel / se_gate_dh_partial_kernel
constexpr int SE_GC = 64;    // channels per split of the dh reduction (its W_up rows: 32 KiB of LDS at R = 128)
constexpr int SE_DN = 8;     // images per workgroup of se_gate_da_kernel

// h[n][r] = relu(sum_c a[n][c] W_down[r][c]): workgroup (16 r's, image n); a wave per r, lanes over c in 16-byte
// pieces, xor-butterfly sum: a fixed order
__global__ __launch_bounds__(256) void se_gate_h_kernel(const float* __restrict__ a, const float* __restrict__ wd, int C,
                                                        int R, float* __restrict__ h) {
  __shared__ float sa[SE_MAX_C];
  const int n = blockIdx.y, r0 = blockIdx.x * 16, t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int c = t; c < C; c += 256) sa[c] = a[(long)n * C + c];
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + 4 * k + w;  // wave-uniform
    if (r >= R) continue;
    float acc = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
      const f32x4 wv = *(const f32x4*)(wd + (long)r * C + c);
      acc = fmaf(sa[c], wv[0], acc);
      acc = fmaf(sa[c + 1], wv[1], acc);
      acc = fmaf(sa[c + 2], wv[2], acc);
      acc = fmaf(sa[c + 3], wv[3], acc);
    }
    acc = fmaxf(warp_sum(acc), 0.f);
    if (lane == 0) h[(long)n * R + r] = acc;
  }
}

// s[n][c] = sigmoid(sum_r h[n][r] W_up[c][r]): workgroup (64 channels, 16 images); the channels' W_up rows are
// staged through LDS (coalesced: they are contiguous), r in order
__global__ __launch_bounds__(256) void se_gate_s_kernel(const float* __restrict__ h, const float* __restrict__ wu, int N,
                                                        int C, int R, float* __restrict__ s) {
  __shared__ float tw[64 * (SE_MAX_R + 1)];
  __shared__ float sh[SE_GN * SE_MAX_R];
  const int c0 = blockIdx.x * 64, n0 = blockIdx.y * SE_GN, t = threadIdx.x;
  const int nn = min(SE_GN, N - n0), cn = min(64, C - c0);
  for (int i = t; i < cn * R; i += 256) tw[(i / R) * (R + 1) + i % R] = wu[(long)c0 * R + i];
  for (int i = t; i < nn * R; i += 256) sh[i] = h[(long)n0 * R + i];
  __syncthreads();
  const int cl = t & 63, nl = t >> 6;
  if (cl >= cn) return;
  for (int n = nl; n < nn; n += 4) {
    float z = 0.f;
    for (int r = 0; r < R; ++r) z = fmaf(sh[n * R + r], tw[cl * (R + 1) + r], z);
    s[(long)(n0 + n) * C + c0 + cl] = 1.0f / (1.0f + expf(-z));
  }
}

// workgroup (channel split ks of SE_GC channels, 16 images; the split's W_up rows staged through LDS): dt =
// (gamma P2 + beta P1) s (1 - s) for its channels
// (written: the weight gradient reads it) and the split's share of dt W_up, part[ks][n][r].  Thread: r = t % Rp
// (Rp: the power of two >= R), image lane g = t / Rp of G = 256 / Rp >= 2: up to 8 images per thread share a
// W_up load.
__global__ __launch_bounds__(256) void se_gate_dh_partial_kernel(const float* __restrict__ p1,
                                                                 const float* __restrict__ p2,
                                                                 const float* __restrict__ s,
                                                                 const float* __restrict__ wu,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int N, int C, int R,
                                                                 int Rp, float* __restrict__ dt,
                                                                 float* __restrict__ part) {
  __shared__ float sdt[SE_GN * SE_GC];
  __shared__ float tw[SE_GC * SE_MAX_R];
  const int ks = blockIdx.x, n0 = blockIdx.y * SE_GN, t = threadIdx.x;
  const int nn = min(SE_GN, N - n0), cA = ks * SE_GC, cn = min(SE_GC, C - cA);
  for (int i = t; i < cn * R; i += 256) tw[i] = wu[(long)cA * R + i];  // the split's rows are contiguous
  for (int i = t; i < nn * cn; i += 256) {
    const int n = i / cn, cl = i - n * cn;
    const long idx = (long)(n0 + n) * C + cA + cl;
    const float ds = gamma[cA + cl] * p2[idx] + beta[cA + cl] * p1[idx];
    const float sg = s[idx];
    const float v = ds * sg * (1.0f - sg);
    sdt[n * SE_GC + cl] = v;
    dt[idx] = v;
  }
  __syncthreads();
  const int G = 256 / Rp, r = t % Rp, g = t / Rp;
  if (r >= R) return;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int cl = 0; cl < cn; ++cl) {
    const float wv = tw[cl * R + r];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = g + j * G;
      if (n < nn) acc[j] = fmaf(sdt[n * SE_GC + cl], wv, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n = g + j * G;
    if (n < nn) part[((long)ks * N + n0 + n) * R + r] = acc[j];
  }
}

// workgroup (256 channels, 8 images): dh = (the splits summed in order) [h > 0] (column 0's workgroups keep it for
// the weight gradient), da[n][c] = sum_r dh[n][r] W_down[r][c], r in order
__global__ __launch_bounds__(256) void se_gate_da_kernel(const float* __restrict__ part, const float* __restrict__ h,
                                                         const float* __restrict__ wd, int N, int C, int R, int KS,
                                                         float* __restrict__ dh, float* __restrict__ da) {
  __shared__ float sdh[SE_DN * SE_MAX_R];
  const int t = threadIdx.x, c = blockIdx.x * 256 + t, n0 = blockIdx.y * SE_DN;
  const int nn = min(SE_DN, N - n0);
  for (int i = t; i < nn * R; i += 256) {
    const long o = (long)n0 * R + i;
    float v = 0.f;
    for (int k = 0; k < KS; ++k) v += part[(long)k * N * R + o];
    v = h[o] > 0.f ? v : 0.f;
    sdh[i] = v;
    if (blockIdx.x == 0) dh[o] = v;
  }
  __syncthreads();
  if (c >= C) return;
  float acc[SE_DN];
#pragma unroll
  for (int j = 0; j < SE_DN; ++j) acc[j] = 0.f;
  for (int r0 = 0; r0 < R; r0 += 8) {  // 8 W_down loads in flight; r in order
    float wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) wv[u] = r0 + u < R ? wd[(long)(r0 + u) * C + c] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (r0 + u >= R) break;
#pragma unroll
      for (int j = 0; j < SE_DN; ++j)
        if (j < nn) acc[j] = fmaf(sdh[j * R + r0 + u], wv[u], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < SE_DN; ++j)
    if (j < nn) da[(long)(n0 + j) * C + c] = acc[j];
}

// dW_up[c][r] = sum_n dt[n][c] h[n][r] (the first C R threads), dW_down[r][c] = sum_n dh[n][r] a[n][c]: n in order
__global__ __launch_bounds__(256) void se_gate_dw_kernel(const float* __restrict__ dt, const float* __restrict__ dh,
                                                         const float* __restrict__ h, const float* __restrict__ a,
                                                         int N, int C, int R, float* __restrict__ dwu,
                                                         float* __restrict__ dwd) {
  const int i = blockIdx.x * 256 + threadIdx.x, CR = C * R;
  if (i >= 2 * CR) return;
  float v = 0.f;
  if (i < CR) {
    const int c = i / R, r = i - c * R;
    for (int n0 = 0; n0 < N; n0 += 8) {  // 16 loads in flight; n in order (an image past N adds 0)
      float x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x[u] = n0 + u < N ? dt[(long)(n0 + u) * C + c] : 0.f;
        y[u] = n0 + u < N ? h[(long)(n0 + u) * R + r] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) v = fmaf(x[u], y[u], v);
    }
    dwu[i] = v;
  } else {
    const int j = i - CR, r = j / C, c = j - r * C;
    for (int n0 = 0; n0 < N; n0 += 8) {
      float x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        x[u] = n0 + u < N ? dh[(long)(n0 + u) * R + r] : 0.f;
        y[u] = n0 + u < N ? a[(long)(n0 + u) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) v = fmaf(x[u], y[u], v);
    }
    dwd[j] = v;
  }
}

// dbeta[c] = sum_n (s P1 + da), dgamma[c] = sum_n (s P2 + da xbar), xbar = (ybar - mean) rstd: a fixed order
__global__ __launch_bounds__(256) void se_bn_param_grads_kernel(const float* __restrict__ p1,
                                                                const float* __restrict__ p2,
                                                                const float* __restrict__ s,
                                                                const float* __restrict__ da,
                                                                const float* __restrict__ ybar,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, int N, int C,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  // 64 channels x 4 image lanes per workgroup: lane l sums images l, l + 4, ... in order, then the lanes in order
  __shared__ float rb[4][64], rg[4][64];
  const int cl = threadIdx.x & 63, l = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  float db = 0.f, dg = 0.f;
  if (c < C) {
    const float mu = mean[c], rs = rstd[c];
    for (int n = l; n < N; n += 4) {
      const long i = (long)n * C + c;
      const float sg = s[i], d = da[i];
      db += fmaf(sg, p1[i], d);
      dg += fmaf(sg, p2[i], d * ((ybar[i] - mu) * rs));
    }
  }
  rb[l][cl] = db;
  rg[l][cl] = dg;
  __syncthreads();
  if (l != 0 || c >= C) return;
  dbeta[c] = (rb[0][cl] + rb[1][cl]) + (rb[2][cl] + rb[3][cl]);
  dgamma[c] = (rg[0][cl] + rg[1][cl]) + (rg[2][cl] + rg[3][cl]);
}

// ---- the two gated BatchNorm apply passes.  Workgroups [n gx, (n + 1) gx) walk image n; gx 256 is a multiple
// of CV = C / VEC, so a thread's channel group -- and with it its BatchNorm parameters and its gate -- never
// changes (bn_apply_cs_kernel's scheme, conv.hip).
// out = relu(s o + res), o = bn_affine(y): BatchNorm's own affine form, the gate and the residual in one fma,
// the result rounded once to the map's type.  With s == 1 that is bn_apply_cs_kernel's (o + res) bit for bit.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void se_apply_kernel(const T* __restrict__ y, const T* __restrict__ res,
                                                       const float* __restrict__ s, int gx, int nvi, int CV,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       T* __restrict__ out) {
  const int n = blockIdx.x / gx, bx = blockIdx.x - n * gx;
  const int t0 = bx * 256 + threadIdx.x, stride = gx * 256;
  const int c = (t0 % CV) * VEC;
  float mu[VEC], rs[VEC], ga[VEC], be[VEC], sg[VEC];
  ldv<VEC>(mean + c, mu);
  ldv<VEC>(rstd + c, rs);
  ldv<VEC>(gamma + c, ga);
  ldv<VEC>(beta + c, be);
  ldv<VEC>(s + (long)n * CV * VEC + c, sg);
  const long base = (long)n * nvi * VEC;
  for (int i = t0; i < nvi; i += stride) {
    const long o = base + (long)i * VEC;
    float xv[VEC], rr[VEC], v[VEC];
    ldv<VEC>(y + o, xv);
    ldv<VEC>(res + o, rr);
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      v[j] = fmaxf(__builtin_fmaf(sg[j], bn_affine(xv[j], mu[j], rs[j], ga[j], be[j]), rr[j]), 0.f);
    stv<VEC>(out + o, v);
  }
}

// dy at one element, rounding pinned (no contraction), in bn_bwd_dx's form (conv.hip):
// d_o = g s + da / HW;  train: dy = (rstd gamma) ((d_o - dbeta / M) - xhat dgamma / M);  eval: (rstd gamma) d_o
__device__ __forceinline__ float se_bwd_dx(float x, float g, float sg, float dam, float mu, float rs, float ga,
                                           float b, float gm, bool train) {
#pragma clang fp contract(off)
  const float d = g * sg + dam;
  if (!train) return (rs * ga) * d;
  const float xh = (x - mu) * rs;
  return (rs * ga) * ((d - b) - xh * gm);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void se_bwd_dx_kernel(const T* __restrict__ y, const T* __restrict__ out,
                                                        const T* __restrict__ dout, const float* __restrict__ s,
                                                        const float* __restrict__ da, int gx, int nvi, int CV, int HW,
                                                        int M, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ dgamma,
                                                        const float* __restrict__ dbeta, int train, T* __restrict__ dy,
                                                        T* __restrict__ gres, int accumulate) {
  const int n = blockIdx.x / gx, bx = blockIdx.x - n * gx;
  const int t0 = bx * 256 + threadIdx.x, stride = gx * 256;
  const int c = (t0 % CV) * VEC;
  float mu[VEC], rs[VEC], ga[VEC], sg[VEC], dam[VEC], b[VEC], gm[VEC];
  ldv<VEC>(mean + c, mu);
  ldv<VEC>(rstd + c, rs);
  ldv<VEC>(gamma + c, ga);
  ldv<VEC>(s + (long)n * CV * VEC + c, sg);
  ldv<VEC>(da + (long)n * CV * VEC + c, dam);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    dam[j] = __fdiv_rn(dam[j], (float)HW);
    b[j] = gm[j] = 0.f;
  }
  if (train) {
    ldv<VEC>(dbeta + c, b);
    ldv<VEC>(dgamma + c, gm);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      b[j] = __fdiv_rn(b[j], (float)M);
      gm[j] = __fdiv_rn(gm[j], (float)M);
    }
  }
  const long base = (long)n * nvi * VEC;
  for (int i = t0; i < nvi; i += stride) {
    const long o = base + (long)i * VEC;
    float xv[VEC], gg[VEC], oo[VEC], v[VEC];
    ldv<VEC>(y + o, xv);
    ldv<VEC>(dout + o, gg);
    ldv<VEC>(out + o, oo);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (!(oo[j] > 0.f)) gg[j] = 0.f;
      v[j] = se_bwd_dx(xv[j], gg[j], sg[j], dam[j], mu[j], rs[j], ga[j], b[j], gm[j], train != 0);
    }
    stv<VEC>(dy + o, v);
    if (accumulate) {
      float prev[VEC];
      ldv<VEC>(gres + o, prev);
#pragma unroll
      for (int j = 0; j < VEC; ++j) gg[j] += prev[j];
    }
    stv<VEC>(gres + o, gg);
  }
}

// train: mean / biased variance from the channel sums (sum x, sum (x - mean)^2), running buffers with the
// unbiased variance, num_batches_tracked += 1 -- chan_final_kernel's FIN 1 / 2 arithmetic (conv.hip);
// eval: mean = running mean, rstd = 1 / sqrt(running_var + eps) correctly rounded (bn_eval_rstd, conv.hip)
__global__ __launch_bounds__(256) void se_bn_stats_kernel(const float* __restrict__ sum, const float* __restrict__ sq,
                                                          int rows, int C, float eps, float momentum, int train,
                                                          float* __restrict__ mean, float* __restrict__ rstd,
                                                          float* __restrict__ run_mean, float* __restrict__ run_var,
                                                          int64_t* __restrict__ nbt) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (train && c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  if (!train) {
    mean[c] = run_mean[c];
    rstd[c] = __fdiv_rn(1.0f, __fsqrt_rn(run_var[c] + eps));
    return;
  }
  const float mu = sum[c] / (float)rows, var = sq[c] / (float)rows;
  mean[c] = mu;
  rstd[c] = 1.0f / sqrtf(var + eps);
  const float unb = rows > 1 ? sq[c] / (float)(rows - 1) : var;
  run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
  run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
}

// ---- host side ----------------------------------------------------------------------------------------------
inline bool se_shape_ok(int N, int HW, int C) {
  return N >= 1 && HW >= 1 && C >= 16 && C <= SE_MAX_C && C % 16 == 0 && (long)HW * C < (1L << 31) &&
         (long)N * C < (1L << 31);
}

// the HW splits of the two sums passes: ~2048 workgroups where the map is large enough, at least four rows per
// row lane and split, at most 64 splits
struct SeSplit {
  int CC, S, per;
};
inline SeSplit se_split(int N, int HW, int C, int VEC) {
  const int CV = C / VEC, cpp = CV < 256 ? CV : 256, rp = 256 / cpp;
  SeSplit sp;
  sp.CC = (CV + cpp - 1) / cpp;
  const long want = (2048 + (long)N * sp.CC - 1) / ((long)N * sp.CC);
  const long most = ((long)HW + 4 * rp - 1) / (4 * rp);
  long S = want < most ? want : most;
  S = S < 1 ? 1 : (S > 64 ? 64 : S);
  sp.per = (int)((HW + S - 1) / S);
  sp.S = (HW + sp.per - 1) / sp.per;
  return sp;
}

// workgroups per image of the apply passes: ~4 vectors per thread, a whole number of channel-group rounds
inline int se_apply_gx(long nvi, int CV) {
  long g = ((nvi + 255) / 256 + 3) / 4;
  if (g < 1) g = 1;
  const int a = CV / std::gcd(CV, 256);
  return (int)((g + a - 1) / a * a);
}
inline bool se_grid_ok(int N, int gx) { return (long)N * gx < (1L << 31); }

template <typename T>
int se_squeeze_impl(const T* y, int N, int HW, int C, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, float* ybar, float* a, float* ws, hipStream_t stream) {
  constexpr int V = MapVec<T>::V;
  const SeSplit sp = se_split(N, HW, C, V);
  if (N > 65535 || sp.CC > 65535) return ES_BAD_SHAPE;
  hipLaunchKernelGGL((se_partial_kernel<T, V, false>), dim3(sp.S, N, sp.CC), 256, 0, stream, y, (const T*)nullptr,
                     (const T*)nullptr, HW, C, sp.per, sp.S, mean, rstd, ws);
  hipLaunchKernelGGL(se_squeeze_final_kernel, (unsigned)(((long)N * C + 255) / 256), 256, 0, stream, ws, N, HW, C,
                     sp.S, mean, rstd, gamma, beta, ybar, a);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int se_sums_impl(const T* y, const T* out, const T* dout, int N, int HW, int C, const float* mean, const float* rstd,
                 float* p1, float* p2, float* ws, hipStream_t stream) {
  constexpr int V = MapVec<T>::V;
  const SeSplit sp = se_split(N, HW, C, V);
  if (N > 65535 || sp.CC > 65535) return ES_BAD_SHAPE;
  hipLaunchKernelGGL((se_partial_kernel<T, V, true>), dim3(sp.S, N, sp.CC), 256, 0, stream, y, out, dout, HW, C,
                     sp.per, sp.S, mean, rstd, ws);
  hipLaunchKernelGGL(se_sums_final_kernel, (unsigned)(((long)N * C + 255) / 256), 256, 0, stream, ws, N, C, sp.S, p1,
                     p2);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int se_apply_impl(const T* y, const T* res, const float* s, int N, int HW, int C, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, T* out, hipStream_t stream) {
  constexpr int V = MapVec<T>::V;
  const int CV = C / V, nvi = HW * CV, gx = se_apply_gx(nvi, CV);
  if (!se_grid_ok(N, gx)) return ES_BAD_SHAPE;
  hipLaunchKernelGGL((se_apply_kernel<T, V>), (unsigned)((long)N * gx), 256, 0, stream, y, res, s, gx, nvi, CV, mean,
                     rstd, gamma, beta, out);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int se_dx_impl(const T* y, const T* out, const T* dout, const float* s, const float* da, int N, int HW, int C,
               const float* mean, const float* rstd, const float* gamma, const float* dgamma, const float* dbeta,
               int train, T* dy, T* gres, int accumulate, hipStream_t stream) {
  constexpr int V = MapVec<T>::V;
  const int CV = C / V, nvi = HW * CV, gx = se_apply_gx(nvi, CV);
  if (!se_grid_ok(N, gx) || (long)N * HW >= (1L << 31)) return ES_BAD_SHAPE;
  hipLaunchKernelGGL((se_bwd_dx_kernel<T, V>), (unsigned)((long)N * gx), 256, 0, stream, y, out, dout, s, da, gx, nvi,
                     CV, HW, N * HW, mean, rstd, gamma, dgamma, dbeta, train, dy, gres, accumulate);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

inline size_t se_partial_floats(int N, int HW, int C, int flags, int width) {
  if (!se_shape_ok(N, HW, C) || (flags & ~SE_MAPS_BF16)) return 0;
  const SeSplit sp = se_split(N, HW, C, flags ? 8 : 4);
  return (size_t)N * sp.S * width * C;
}

}  // namespace

extern "C" {

// floats of workspace for es_se_squeeze_ex / es_se_bn_bwd_sums_ex (0 for an unsupported shape)
size_t es_se_squeeze_workspace(int N, int HW, int C, int flags) { return se_partial_floats(N, HW, C, flags, 1); }
size_t es_se_bn_bwd_sums_workspace(int N, int HW, int C, int flags) { return se_partial_floats(N, HW, C, flags, 2); }
// floats of workspace for es_se_gate_bwd: dt [N, C], dh [N, R] and the dh reduction's splits [C / 128][N, R]
size_t es_se_gate_bwd_workspace(int N, int C, int R) {
  if (N < 1 || C < 16 || C > SE_MAX_C || C % 16 || R < 1 || R > SE_MAX_R) return 0;
  const size_t KS = (C + SE_GC - 1) / SE_GC;
  return (size_t)N * C + (((size_t)N * R + 3) & ~(size_t)3) + KS * N * R;
}

int es_se_bn_stats(const float* sum, const float* sq, int rows, int C, float eps, float momentum, int train,
                   float* mean, float* rstd, float* running_mean, float* running_var, void* num_batches_tracked,
                   hipStream_t stream) {
  if (!mean || !rstd || !running_mean || !running_var || (train && (!sum || !sq))) return ES_BAD_ARG;
  if (rows < 1 || C < 1) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(se_bn_stats_kernel, (C + 255) / 256, 256, 0, stream, sum, sq, rows, C, eps, momentum, train, mean,
                     rstd, running_mean, running_var, (int64_t*)num_batches_tracked);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_se_squeeze_ex(const void* y, int N, int HW, int C, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float* ybar, float* a, float* workspace, int flags, hipStream_t stream) {
  if (flags & ~SE_MAPS_BF16) return ES_BAD_ARG;
  if (!y || !mean || !rstd || !gamma || !beta || !ybar || !a || !workspace) return ES_BAD_ARG;
  if (!al16(y)) return ES_BAD_ARG;
  if (!se_shape_ok(N, HW, C)) return ES_BAD_SHAPE;
  return flags ? se_squeeze_impl<bf16>((const bf16*)y, N, HW, C, mean, rstd, gamma, beta, ybar, a, workspace, stream)
               : se_squeeze_impl<float>((const float*)y, N, HW, C, mean, rstd, gamma, beta, ybar, a, workspace,
                                        stream);
}

int es_se_gate_fwd(const float* a, const float* w_down, const float* w_up, int N, int C, int R, float* h, float* s,
                   hipStream_t stream) {
  if (!a || !w_down || !w_up || !h || !s) return ES_BAD_ARG;
  if (!al16(w_down)) return ES_BAD_ARG;
  if (!se_shape_ok(N, 1, C) || R < 1 || R > SE_MAX_R || N > 65535) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(se_gate_h_kernel, dim3((R + 15) / 16, N), 256, 0, stream, a, w_down, C, R, h);
  hipLaunchKernelGGL(se_gate_s_kernel, dim3((C + 63) / 64, (N + SE_GN - 1) / SE_GN), 256, 0, stream, h, w_up, N, C, R,
                     s);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_se_bn_apply_ex(const void* y, const void* res, const float* s, int N, int HW, int C, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, void* out, int flags,
                      hipStream_t stream) {
  if (flags & ~SE_MAPS_BF16) return ES_BAD_ARG;
  if (!y || !res || !s || !mean || !rstd || !gamma || !beta || !out) return ES_BAD_ARG;
  if (!al16(y) || !al16(res) || !al16(out) || !al16(s) || !al16(mean) || !al16(rstd) || !al16(gamma) || !al16(beta))
    return ES_BAD_ARG;
  if (!se_shape_ok(N, HW, C)) return ES_BAD_SHAPE;
  return flags ? se_apply_impl<bf16>((const bf16*)y, (const bf16*)res, s, N, HW, C, mean, rstd, gamma, beta,
                                     (bf16*)out, stream)
               : se_apply_impl<float>((const float*)y, (const float*)res, s, N, HW, C, mean, rstd, gamma, beta,
                                      (float*)out, stream);
}

int es_se_bn_bwd_sums_ex(const void* y, const void* out, const void* dout, int N, int HW, int C, const float* mean,
                         const float* rstd, float* p1, float* p2, float* workspace, int flags, hipStream_t stream) {
  if (flags & ~SE_MAPS_BF16) return ES_BAD_ARG;
  if (!y || !out || !dout || !mean || !rstd || !p1 || !p2 || !workspace) return ES_BAD_ARG;
  if (!al16(y) || !al16(out) || !al16(dout) || !al16(mean) || !al16(rstd)) return ES_BAD_ARG;
  if (!se_shape_ok(N, HW, C)) return ES_BAD_SHAPE;
  return flags ? se_sums_impl<bf16>((const bf16*)y, (const bf16*)out, (const bf16*)dout, N, HW, C, mean, rstd, p1, p2,
                                    workspace, stream)
               : se_sums_impl<float>((const float*)y, (const float*)out, (const float*)dout, N, HW, C, mean, rstd, p1,
                                     p2, workspace, stream);
}

int es_se_gate_bwd(const float* p1, const float* p2, const float* ybar, const float* a, const float* h,
                   const float* s, const float* w_down, const float* w_up, const float* gamma, const float* beta,
                   const float* mean, const float* rstd, int N, int C, int R, float* dw_down, float* dw_up, float* da,
                   float* dgamma, float* dbeta, float* workspace, hipStream_t stream) {
  if (!p1 || !p2 || !ybar || !a || !h || !s || !w_down || !w_up || !gamma || !beta || !mean || !rstd || !dw_down ||
      !dw_up || !da || !dgamma || !dbeta || !workspace)
    return ES_BAD_ARG;
  if (!se_shape_ok(N, 1, C) || R < 1 || R > SE_MAX_R) return ES_BAD_SHAPE;
  const int KS = (C + SE_GC - 1) / SE_GC;
  float* dt = workspace;
  float* dh = workspace + (size_t)N * C;
  float* part = dh + (((size_t)N * R + 3) & ~(size_t)3);
  int Rp = 1;
  while (Rp < R) Rp <<= 1;
  hipLaunchKernelGGL(se_gate_dh_partial_kernel, dim3(KS, (N + SE_GN - 1) / SE_GN), 256, 0, stream, p1, p2, s, w_up,
                     gamma, beta, N, C, R, Rp, dt, part);
  hipLaunchKernelGGL(se_gate_da_kernel, dim3((C + 255) / 256, (N + SE_DN - 1) / SE_DN), 256, 0, stream, part, h,
                     w_down, N, C, R, KS, dh, da);
  hipLaunchKernelGGL(se_gate_dw_kernel, (2 * C * R + 255) / 256, 256, 0, stream, dt, dh, h, a, N, C, R, dw_up,
                     dw_down);
  hipLaunchKernelGGL(se_bn_param_grads_kernel, (C + 63) / 64, 256, 0, stream, p1, p2, s, da, ybar, mean, rstd, N, C,
                     dgamma, dbeta);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_se_bn_bwd_dx_ex(const void* y, const void* out, const void* dout, const float* s, const float* da, int N,
                       int HW, int C, const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                       const float* dbeta, int train, void* dy, void* gres, int accumulate, int flags,
                       hipStream_t stream) {
  if (flags & ~SE_MAPS_BF16) return ES_BAD_ARG;
  if (!y || !out || !dout || !s || !da || !mean || !rstd || !gamma || !dy || !gres || (train && (!dgamma || !dbeta)))
    return ES_BAD_ARG;
  if (!al16(y) || !al16(out) || !al16(dout) || !al16(dy) || !al16(gres) || !al16(s) || !al16(da) || !al16(mean) ||
      !al16(rstd) || !al16(gamma) || (train && (!al16(dgamma) || !al16(dbeta))))
    return ES_BAD_ARG;
  if (!se_shape_ok(N, HW, C)) return ES_BAD_SHAPE;
  return flags ? se_dx_impl<bf16>((const bf16*)y, (const bf16*)out, (const bf16*)dout, s, da, N, HW, C, mean, rstd,
                                  gamma, dgamma, dbeta, train, (bf16*)dy, (bf16*)gres, accumulate, stream)
               : se_dx_impl<float>((const float*)y, (const float*)out, (const float*)dout, s, da, N, HW, C, mean, rstd,
                                   gamma, dgamma, dbeta, train, (float*)dy, (float*)gres, accumulate, stream);
}

}  // extern "C"
