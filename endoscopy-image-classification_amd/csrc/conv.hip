// CNN-branch kernels of the Conformer (SemiFormer's backbone):
// code/models/conformer.py:75-445 -- ConvBlock / Med_ConvBlock / FCUDown / FCUUp / stem.
//
//  es_conv2d_fwd / _bwd_data / _bwd_weight   Conv2d (groups = 1) as an fp32 implicit GEMM over
//                                            NHWC maps with element strides (so the first conv
//                                            reads the NCHW images and the FCU convs read / write
//                                            token rows of the transformer buffer directly)
//  es_chan_sum                               per-channel sums (bias gradients)
//  es_bn2d_fwd / es_bn2d_bwd                 BatchNorm2d (train: batch statistics + running
//                                            update; eval: running statistics), fused residual
//                                            add and ReLU (ConvBlock's bn3 + residual + act3)
//  es_maxpool2d_fwd / _bwd                   MaxPool2d(k, s, p), first maximum wins (torch CPU)
//  es_avgpool2d_fwd / _bwd                   AvgPool2d(k, k) (FCUDown) and AdaptiveAvgPool2d(1)
//  es_upsample_add_fwd / _bwd                x + interpolate(x_t, nearest, x s) (FCUUp -> conv2)
//  es_fcu_down_tokens_fwd / _bwd             FCUDown's LayerNorm + GELU + cat(cls) and the
//                                            `x_st + x_t` of ConvTransBlock.forward (:345-346)
//  es_tokens_cls_set                         x_t[:, 0] = cls_token (Conformer.forward :422-429)
//
// MI355X notes: the CNN branch of Conformer-Ti is ~0.7 GMAC per image against the transformer
// branch's ~4.6, and its tensors are small-channel (16..256) maps, so these kernels are fp32 SIMT
// implicit GEMMs (64x64 / 128x32 / 256x16 output tiles, 4x4 per thread, 16-deep K steps staged
// through LDS) -- no bf16 rounding on the BatchNorm-coupled CNN path (BatchNorm over the whole
// batch amplifies operand noise, the same effect as CoMatch's BatchNorm1d head).
#include <numeric>

#include "common.h"
#include "bn_rows.h"

namespace {

struct ConvGeom {
  int N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad;
  long sxn, sxh, sxw, sxc;  // input element strides (n, h, w, c)
  long syn, syh, syw;       // output strides (channel stride 1)
};

constexpr int CBK = 16;

// Every implicit-GEMM kernel below runs 256 threads over a 16-deep K (or pixel) step.  The gathers
// avoid per-element integer division: a thread's K lane (ki = tid & 15) is fixed, so its (ci, kx, ky)
// decomposition is advanced incrementally by 16 per step; its rows' (n, h, w) decompositions are
// computed once before the K loop.

// k -> (c, kx, ky) with c fastest (NHWC-contiguous gathers), advanced by `step` per K step
struct KWalk {
  int c, kx, ky, t2;  // t2 = ky * kw + kx
  __device__ void init(int k, int C, int kw) {
    c = k % C;
    t2 = k / C;
    kx = t2 % kw;
    ky = t2 / kw;
  }
  __device__ void advance(int step, int C, int kw) {
    c += step;
    while (c >= C) {
      c -= C;
      ++t2;
      if (++kx == kw) {
        kx = 0;
        ++ky;
      }
    }
  }
};

// fp32 MFMA tile engine over the k-major LDS tiles As[CBK][BM + 1] (GEMM rows) and Bs[CBK][BN + 4]
// (GEMM cols) that every kernel below stages: 4 waves as WM x WN, wave tile MF x NF tiles of 16x16,
// v_mfma_f32_16x16x4_f32 (lane l: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; D col l & 15, row
// 4 (l >> 4) + q).  That instruction is bit for bit a k-ordered f32 fmaf chain (MI355X_MICROARCH.md
// FP32-input MFMA), so results equal the SIMT fmaf loop's while the matrix cores do the arithmetic
// and the VALU is left to the im2col gathers.
template <int BM, int BN>
struct ConvMfma {
  static constexpr int WM = BM < 32 ? 1 : (BN < 32 ? 4 : 2), WN = 4 / WM;
  static constexpr int MF = BM / (WM * 16), NF = BN / (WN * 16);
  static_assert(MF >= 1 && NF >= 1 && MF * WM * 16 == BM && NF * WN * 16 == BN, "conv MFMA tile");
  f32x4 acc[MF][NF];
  int rb, cb, lr, lk;  // wave's first row / col in the tile, lane's row-in-16 / k-in-4
  __device__ __forceinline__ void init() {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    rb = (w / WN) * MF * 16;
    cb = (w % WN) * NF * 16;
    lr = lane & 15;
    lk = lane >> 4;
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void step(const float (*As)[BM + 1], const float (*Bs)[BN + 4]) {
#pragma unroll
    for (int kk = 0; kk < CBK; kk += 4) {
      float a[MF], b[NF];
#pragma unroll
      for (int i = 0; i < MF; ++i) a[i] = As[kk + lk][rb + i * 16 + lr];
#pragma unroll
      for (int j = 0; j < NF; ++j) b[j] = Bs[kk + lk][cb + j * 16 + lr];
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // tile-relative coordinates of acc[i][j][q]
  __device__ __forceinline__ int row(int i, int q) const { return rb + i * 16 + 4 * lk + q; }
  __device__ __forceinline__ int col(int j) const { return cb + j * 16 + lr; }
};

// ---- forward: y[n,ho,wo,co] = bias[co] + sum_{ky,kx,ci} x[n, ho*s-p+ky, wo*s-p+kx, ci] w[co,ci,ky,kx]
// GEMM rows m = (n, ho, wo), cols co, K = (ky, kx, ci).  VEC = 4 (Cin % 4 == 0, channel-contiguous
// 16-byte aligned pixels): the im2col gather loads 4 channels of one tap per instruction (threads =
// 4 channel quads x 64 rows); VEC = 1: one channel per thread (16 k x 16 rows).
template <int BM, int BN, int VEC>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y,
                                                       ConvGeom g, int accumulate) {
  constexpr int RSTEP = 256 / (CBK / VEC);  // rows per gather pass
  constexpr int APR = BM / RSTEP, BPR = BN / 16;
  static_assert(BM % RSTEP == 0, "gather rows");
  __shared__ float As[CBK][BM + 1];
  __shared__ float Bs[CBK][BN + 4];
  const int M = g.N * g.Ho * g.Wo, K = g.kh * g.kw * g.Cin, KK = g.kh * g.kw;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int ki = tid & 15, r16 = tid >> 4;                        // weight gather
  const int ka = (tid % (CBK / VEC)) * VEC, ra = tid / (CBK / VEC);  // image gather
  long abase[APR];
  int ahb[APR], awb[APR];
#pragma unroll
  for (int j = 0; j < APR; ++j) {
    const int m = m0 + ra + RSTEP * j;
    if (m < M) {
      const int wo = m % g.Wo, t = m / g.Wo, ho = t % g.Ho, n = t / g.Ho;
      abase[j] = n * g.sxn;
      ahb[j] = ho * g.stride - g.pad;
      awb[j] = wo * g.stride - g.pad;
    } else {
      abase[j] = 0;
      ahb[j] = -(1 << 28);
      awb[j] = 0;
    }
  }
  long bbase[BPR];
#pragma unroll
  for (int j = 0; j < BPR; ++j) {
    const int co = n0 + r16 + 16 * j;
    bbase[j] = co < g.Cout ? (long)co * g.Cin * KK : -1;
  }
  KWalk kw, kwa;
  kw.init(ki, g.Cin, g.kw);
  kwa.init(ka, g.Cin, g.kw);
  ConvMfma<BM, BN> mt;
  mt.init();
  for (int k0 = 0; k0 < K; k0 += CBK) {
    const bool kok = k0 + ki < K, koka = k0 + ka < K;
#pragma unroll
    for (int j = 0; j < APR; ++j) {
      const int h = ahb[j] + kwa.ky, ww = awb[j] + kwa.kx;
      const bool ok = koka && (unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W;
      if constexpr (VEC == 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *(const f32x4*)(x + abase[j] + h * g.sxh + ww * g.sxw + kwa.c);
#pragma unroll
        for (int e = 0; e < 4; ++e) As[ka + e][ra + RSTEP * j] = v[e];
      } else {
        As[ka][ra + RSTEP * j] = ok ? x[abase[j] + h * g.sxh + ww * g.sxw + kwa.c * g.sxc] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < BPR; ++j)
      Bs[ki][r16 + 16 * j] = (kok && bbase[j] >= 0) ? w[bbase[j] + (long)kw.c * KK + kw.t2] : 0.f;
    kw.advance(CBK, g.Cin, g.kw);
    kwa.advance(CBK, g.Cin, g.kw);
    __syncthreads();
    mt.step(As, Bs);
    __syncthreads();
  }
  float bv[ConvMfma<BM, BN>::NF];
#pragma unroll
  for (int j = 0; j < ConvMfma<BM, BN>::NF; ++j) {
    const int co = n0 + mt.col(j);
    bv[j] = (bias && co < g.Cout) ? bias[co] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < ConvMfma<BM, BN>::MF; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + mt.row(i, q);
      if (m >= M) continue;
      const int wo = m % g.Wo, t = m / g.Wo, ho = t % g.Ho, n = t / g.Ho;
      float* yr = y + n * g.syn + ho * g.syh + wo * g.syw;
#pragma unroll
      for (int j = 0; j < ConvMfma<BM, BN>::NF; ++j) {
        const int co = n0 + mt.col(j);
        if (co < g.Cout) {
          const float v = mt.acc[i][j][q] + bv[j];
          yr[co] = accumulate ? yr[co] + v : v;
        }
      }
    }
}

// ---- data gradient: dx[n,h,w,ci] (+)= sum_{ky,kx,co} dy[n,ho,wo,co] w[co,ci,ky,kx],
// ho = (h + p - ky) / s when divisible and in range.  Split by stride phase: blockIdx.z = (py, px)
// takes the pixels h = hq*s + py, w = wq*s + px, whose only valid taps are ky = ky0 + s*kyq with
// ky0 = (py + p) mod s (likewise kx), so ho = hq + (py + p - ky0)/s - kyq exactly.  Rows m = (n, hq, wq)
// of the phase, cols ci, K = (kyq, kxq, co): no tap is visited that the stride makes invalid (the
// strided patch conv k = s = 4 would otherwise waste 15/16 of its K loop).  VEC = 4 (Cout % 4 == 0,
// 16-byte aligned dy rows): 4 output channels of one tap per gather load, as in conv_fwd_kernel.
template <int BM, int BN, int VEC>
__global__ __launch_bounds__(256) void conv_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                      float* __restrict__ dx, ConvGeom g, int accumulate) {
  constexpr int RSTEP = 256 / (CBK / VEC);
  constexpr int APR = BM / RSTEP, BPR = BN / 16;
  static_assert(BM % RSTEP == 0, "gather rows");
  __shared__ float As[CBK][BM + 1];
  __shared__ float Bs[CBK][BN + 4];
  const int s = g.stride;
  const int py = blockIdx.z / s, px = blockIdx.z - py * s;
  const int Hq = (g.H - py + s - 1) / s, Wq = (g.W - px + s - 1) / s;
  const int ky0 = (py + g.pad) % s, kx0 = (px + g.pad) % s;
  const int khq = g.kh > ky0 ? (g.kh - ky0 + s - 1) / s : 0, kwq = g.kw > kx0 ? (g.kw - kx0 + s - 1) / s : 0;
  const int qh = (py + g.pad - ky0) / s, qw = (px + g.pad - kx0) / s;
  const int M = g.N * Hq * Wq, K = khq * kwq * g.Cout, KK = g.kh * g.kw;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  if (m0 >= M) return;  // this phase has fewer pixels (block-uniform)
  const int tid = threadIdx.x;
  const int ki = tid & 15, r16 = tid >> 4;
  const int ka = (tid % (CBK / VEC)) * VEC, ra = tid / (CBK / VEC);
  long abase[APR];
  int ahq[APR], awq[APR];
#pragma unroll
  for (int j = 0; j < APR; ++j) {
    const int m = m0 + ra + RSTEP * j;
    if (m < M) {
      const int wq = m % Wq, t = m / Wq, hq = t % Hq, n = t / Hq;
      abase[j] = n * g.syn;
      ahq[j] = hq + qh;
      awq[j] = wq + qw;
    } else {
      abase[j] = 0;
      ahq[j] = -(1 << 28);
      awq[j] = 0;
    }
  }
  int bci[BPR];
#pragma unroll
  for (int j = 0; j < BPR; ++j) bci[j] = n0 + r16 + 16 * j;
  KWalk kw, kwa;  // (c, kx = kxq, ky = kyq) over the phase's taps
  if (K > 0) {
    kw.init(ki, g.Cout, kwq);
    kwa.init(ka, g.Cout, kwq);
  }
  ConvMfma<BM, BN> mt;
  mt.init();
  for (int k0 = 0; k0 < K; k0 += CBK) {
    const bool kok = k0 + ki < K, koka = k0 + ka < K;
#pragma unroll
    for (int j = 0; j < APR; ++j) {
      const int ho = ahq[j] - kwa.ky, wo = awq[j] - kwa.kx;
      const bool ok = koka && (unsigned)ho < (unsigned)g.Ho && (unsigned)wo < (unsigned)g.Wo;
      if constexpr (VEC == 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *(const f32x4*)(dy + abase[j] + ho * g.syh + wo * g.syw + kwa.c);
#pragma unroll
        for (int e = 0; e < 4; ++e) As[ka + e][ra + RSTEP * j] = v[e];
      } else {
        As[ka][ra + RSTEP * j] = ok ? dy[abase[j] + ho * g.syh + wo * g.syw + kwa.c] : 0.f;
      }
    }
    const int tap = (ky0 + kw.ky * s) * g.kw + kx0 + kw.kx * s;
#pragma unroll
    for (int j = 0; j < BPR; ++j)
      Bs[ki][r16 + 16 * j] = (kok && bci[j] < g.Cin) ? w[((long)kw.c * g.Cin + bci[j]) * KK + tap] : 0.f;
    kw.advance(CBK, g.Cout, kwq);
    kwa.advance(CBK, g.Cout, kwq);
    __syncthreads();
    mt.step(As, Bs);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < ConvMfma<BM, BN>::MF; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + mt.row(i, q);
      if (m >= M) continue;
      const int wq = m % Wq, t = m / Wq, hq = t % Hq, n = t / Hq;
      float* xr = dx + n * g.sxn + (hq * s + py) * g.sxh + (wq * s + px) * g.sxw;
#pragma unroll
      for (int j = 0; j < ConvMfma<BM, BN>::NF; ++j) {
        const int ci = n0 + mt.col(j);
        if (ci < g.Cin) {
          float* p = xr + ci * g.sxc;
          *p = accumulate ? *p + mt.acc[i][j][q] : mt.acc[i][j][q];
        }
      }
    }
}

// pixel index m -> (n, ho, wo), advanced by d (small) without division
struct PWalk {
  int n, ho, wo;
  __device__ void init(int m, int Ho, int Wo) {
    wo = m % Wo;
    const int t = m / Wo;
    ho = t % Ho;
    n = t / Ho;
  }
  __device__ void advance(int d, int Ho, int Wo) {
    wo += d;
    while (wo >= Wo) {
      wo -= Wo;
      if (++ho == Ho) {
        ho = 0;
        ++n;
      }
    }
  }
};

// ---- weight gradient partials: P[split][co][k'] = sum_{m in split} dy[m, co] A[m, k'],
// k' = (ci, ky, kx) (the weight's own layout), A = im2col(x).  Rows co, cols k', reduction over the
// output pixels m of this split (16 per step).  A thread owns one co column of the dy tile and one k'
// column of the im2col tile; its pixels are walked incrementally.
template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      float* __restrict__ P, ConvGeom g, int mchunk) {
  constexpr int AROWS = 256 / BM, APR = 16 / AROWS;  // dy tile: pixel rows per pass, passes
  constexpr int BROWS = 256 / BN, BPR = 16 / BROWS;  // im2col tile
  __shared__ float As[CBK][BM + 1];  // dy^T  [m][co]
  __shared__ float Bs[CBK][BN + 4];  // im2col [m][k']
  const int M = g.N * g.Ho * g.Wo, KK = g.kh * g.kw, K = g.Cin * KK;
  const int c0 = blockIdx.x * BM, n0 = blockIdx.y * BN, split = blockIdx.z;
  const int mb = split * mchunk, me = min(mb + mchunk, M);
  const int tid = threadIdx.x;
  const int aco = c0 + tid % BM, arow = tid / BM;
  // im2col columns in (ky, kx, ci) order, ci fastest: neighbouring threads gather neighbouring
  // channels of one pixel (NHWC-contiguous); the epilogue maps a column back to the weight's
  // (ci, ky, kx) index
  const int bk = n0 + tid % BN, brow = tid / BN;
  int bci = 0, bky = 0, bkx = 0;
  const bool bkok = bk < K;
  if (bkok) {
    bci = bk % g.Cin;
    const int t2 = bk / g.Cin;
    bkx = t2 % g.kw;
    bky = t2 / g.kw;
  }
  PWalk pa[APR], pb[BPR];
#pragma unroll
  for (int j = 0; j < APR; ++j) pa[j].init(mb + arow + AROWS * j, g.Ho, g.Wo);
#pragma unroll
  for (int j = 0; j < BPR; ++j) pb[j].init(mb + brow + BROWS * j, g.Ho, g.Wo);
  ConvMfma<BM, BN> mt;
  mt.init();
  for (int mm = mb; mm < me; mm += CBK) {
#pragma unroll
    for (int j = 0; j < APR; ++j) {
      const int m = mm + arow + AROWS * j;
      float v = 0.f;
      if (m < me && aco < g.Cout) v = dy[pa[j].n * g.syn + pa[j].ho * g.syh + pa[j].wo * g.syw + aco];
      As[arow + AROWS * j][tid % BM] = v;
      pa[j].advance(CBK, g.Ho, g.Wo);
    }
#pragma unroll
    for (int j = 0; j < BPR; ++j) {
      const int m = mm + brow + BROWS * j;
      float v = 0.f;
      if (m < me && bkok) {
        const int h = pb[j].ho * g.stride - g.pad + bky, ww = pb[j].wo * g.stride - g.pad + bkx;
        if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W)
          v = x[pb[j].n * g.sxn + h * g.sxh + ww * g.sxw + bci * g.sxc];
      }
      Bs[brow + BROWS * j][tid % BN] = v;
      pb[j].advance(CBK, g.Ho, g.Wo);
    }
    __syncthreads();
    mt.step(As, Bs);
    __syncthreads();
  }
  float* out = P + (long)split * g.Cout * K;
#pragma unroll
  for (int i = 0; i < ConvMfma<BM, BN>::MF; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = c0 + mt.row(i, q);
      if (co >= g.Cout) continue;
#pragma unroll
      for (int j = 0; j < ConvMfma<BM, BN>::NF; ++j) {
        const int kc = n0 + mt.col(j);  // (ky, kx, ci) column -> weight index ci * KK + ky * kw + kx
        if (kc < K) out[(long)co * K + (kc % g.Cin) * KK + kc / g.Cin] = mt.acc[i][j][q];
      }
    }
}

// out[i] (+)= sum_s P[s][i]
__global__ void sum_slabs_kernel(const float* __restrict__ P, float* __restrict__ out, int S, long n, int accumulate) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float s0 = 0.f, s1 = 0.f;
    int k = 0;
    for (; k + 2 <= S; k += 2) {
      s0 += P[(long)k * n + i];
      s1 += P[(long)(k + 1) * n + i];
    }
    if (k < S) s0 += P[(long)k * n + i];
    const float v = s0 + s1;
    out[i] = accumulate ? out[i] + v : v;
  }
}


// y = (x - mean) * rstd * gamma + beta (+ res) (relu); eval: rstd from the running variance.
// nv = elements / VEC, CV = C / VEC (32-bit index arithmetic: the host checks nv < 2^31)
// T: element type of the maps x, res, y (bf16 maps: widened on load, the result rounded once)
template <int VEC, typename T = float>
__global__ void bn_apply_kernel(const T* __restrict__ x, int nv, int CV, const float* __restrict__ mean,
                                const float* __restrict__ rstd, const float* __restrict__ rvar, float eps,
                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                const T* __restrict__ res, int relu, T* __restrict__ y) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gridDim.x * blockDim.x) {
    const int c = (int)((unsigned)i % (unsigned)CV) * VEC;
    float xv[VEC], mu[VEC], ga[VEC], be[VEC], rs[VEC], rv[VEC], o[VEC];
    ldv<VEC>(x + (long)i * VEC, xv);
    ldv<VEC>(mean + c, mu);
    ldv<VEC>(gamma + c, ga);
    ldv<VEC>(beta + c, be);
    if (rvar) {
      ldv<VEC>(rvar + c, rv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) rs[j] = bn_eval_rstd(rv[j], eps);
    } else {
      ldv<VEC>(rstd + c, rs);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_affine(xv[j], mu[j], rs[j], ga[j], be[j]);
    if (res) {
      float rr[VEC];
      ldv<VEC>(res + (long)i * VEC, rr);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] += rr[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = fmaxf(o[j], 0.f);
    }
    stv<VEC>(y + (long)i * VEC, o);
  }
}

// dx = rstd * gamma * (g - sum(g)/P - xhat * sum(g xhat)/P); g = dy [* (y > 0)] (written to gout
// when given: the residual branch's gradient)
// REBUILD (relu): the mask rebuilt from x with beta (bn_relu_live), y not read
template <int VEC, typename T = float, bool REBUILD = false>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                    const T* __restrict__ y, int relu, int nv, int CV, int rows,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const float* __restrict__ gamma, const float* __restrict__ sums,
                                    T* __restrict__ dx, T* __restrict__ gout, const float* __restrict__ beta = nullptr) {
  const float inv = 1.0f / (float)rows;
  const int C = CV * VEC;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gridDim.x * blockDim.x) {
    const int c = (int)((unsigned)i % (unsigned)CV) * VEC;
    float xv[VEC], gg[VEC], yy[VEC], mu[VEC], rs[VEC], ga[VEC], s0[VEC], s1[VEC], o[VEC];
    ldv<VEC>(x + (long)i * VEC, xv);
    ldv<VEC>(dy + (long)i * VEC, gg);
    if constexpr (REBUILD) {
      float mu0[VEC], rs0[VEC], ga0[VEC], be[VEC];
      ldv<VEC>(mean + c, mu0);
      ldv<VEC>(rstd + c, rs0);
      ldv<VEC>(gamma + c, ga0);
      ldv<VEC>(beta + c, be);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (!bn_relu_live<T>(xv[j], mu0[j], rs0[j], ga0[j], be[j])) gg[j] = 0.f;
    } else if (relu) {
      ldv<VEC>(y + (long)i * VEC, yy);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (!(yy[j] > 0.f)) gg[j] = 0.f;
    }
    if (gout) stv<VEC>(gout + (long)i * VEC, gg);
    ldv<VEC>(mean + c, mu);
    ldv<VEC>(rstd + c, rs);
    ldv<VEC>(gamma + c, ga);
    ldv<VEC>(sums + c, s0);
    ldv<VEC>(sums + C + c, s1);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_bwd_dx(xv[j], gg[j], mu[j], rs[j], ga[j], s0[j], s1[j], inv);
    stv<VEC>(dx + (long)i * VEC, o);
  }
}

// Channel-stationary forms of bn_apply_kernel / bn_bwd_apply_kernel: the launch makes the grid's thread count a
// multiple of CV = C / VEC, so a thread's channel group never changes -- its BatchNorm parameters are loaded once
// instead of every iteration (with an integer modulo by a run-time value), and VEC = 8 on bf16 maps gives 16-byte
// accesses.  The same arithmetic per element: bit-identical maps.
template <int VEC, typename T>
__global__ __launch_bounds__(256) void bn_apply_cs_kernel(const T* __restrict__ x, int nv, int CV,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ rvar, float eps,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const T* __restrict__ res,
                                                          int relu, T* __restrict__ y) {
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const int c = (t0 % CV) * VEC;
  float mu[VEC], ga[VEC], be[VEC], rs[VEC];
  ldv<VEC>(mean + c, mu);
  ldv<VEC>(gamma + c, ga);
  ldv<VEC>(beta + c, be);
  if (rvar) {
    float rv[VEC];
    ldv<VEC>(rvar + c, rv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) rs[j] = bn_eval_rstd(rv[j], eps);
  } else {
    ldv<VEC>(rstd + c, rs);
  }
  for (int i = t0; i < nv; i += stride) {
    float xv[VEC], o[VEC];
    ldv<VEC>(x + (long)i * VEC, xv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_affine(xv[j], mu[j], rs[j], ga[j], be[j]);
    if (res) {
      float rr[VEC];
      ldv<VEC>(res + (long)i * VEC, rr);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] += rr[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = fmaxf(o[j], 0.f);
    }
    stv<VEC>(y + (long)i * VEC, o);
  }
}

template <int VEC, typename T, bool REBUILD = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_cs_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                              const T* __restrict__ y, int relu, int nv, int CV, int rows,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ sums, T* __restrict__ dx,
                                                              T* __restrict__ gout, const float* __restrict__ beta) {
  const float inv = 1.0f / (float)rows;
  const int C = CV * VEC;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const int c = (t0 % CV) * VEC;
  float mu[VEC], rs[VEC], ga[VEC], s0[VEC], s1[VEC], be[VEC];
  ldv<VEC>(mean + c, mu);
  ldv<VEC>(rstd + c, rs);
  ldv<VEC>(gamma + c, ga);
  ldv<VEC>(sums + c, s0);
  ldv<VEC>(sums + C + c, s1);
  if constexpr (REBUILD) ldv<VEC>(beta + c, be);
  for (int i = t0; i < nv; i += stride) {
    float xv[VEC], gg[VEC], o[VEC];
    ldv<VEC>(x + (long)i * VEC, xv);
    ldv<VEC>(dy + (long)i * VEC, gg);
    if constexpr (REBUILD) {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (!bn_relu_live<T>(xv[j], mu[j], rs[j], ga[j], be[j])) gg[j] = 0.f;
    } else if (relu) {
      float yy[VEC];
      ldv<VEC>(y + (long)i * VEC, yy);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (!(yy[j] > 0.f)) gg[j] = 0.f;
    }
    if (gout) stv<VEC>(gout + (long)i * VEC, gg);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = bn_bwd_dx(xv[j], gg[j], mu[j], rs[j], ga[j], s0[j], s1[j], inv);
    stv<VEC>(dx + (long)i * VEC, o);
  }
}

// the channel-stationary grid: ~16,384 workgroups at most, thread count a multiple of CV
inline int cs_grid(long nv, int CV) {
  const long b = (nv + 255) / 256;
  int g = (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));  // grid1d's cap
  const int a = CV / std::gcd(CV, 256);  // workgroups per whole number of channel groups
  g = (g + a - 1) / a * a;
  return g;
}
int g_bn_cs = 1;  // es_set_bn_cs: the channel-stationary BatchNorm applies (0: the per-iteration forms)
int g_bn_sum8 = 0;  // es_set_bn_sum8: 8-channel groups in the BatchNorm channel sums (a test knob: another order)

// eval-mode BatchNorm backward is an affine map: dx = g * gamma * rstd_running (not on the training
// path; kept for completeness of the autograd surface)
template <typename T = float>
__global__ void bn_bwd_eval_kernel(const T* __restrict__ dy, const T* __restrict__ y, int relu, long n, int C,
                                   const float* __restrict__ rvar, float eps, const float* __restrict__ gamma,
                                   T* __restrict__ dx, T* __restrict__ gout) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    float gg = m_f32(dy[i]);
    if (relu && !(m_f32(y[i]) > 0.f)) gg = 0.f;
    if (gout) m_store(gout + i, gg);
    m_store(dx + i, gg * gamma[c] / sqrtf(rvar[c] + eps));
  }
}

// ---- pooling / upsampling (NHWC contiguous)
template <typename TO = float>
__global__ void maxpool_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, int k, int s, int p,
                                   int Ho, int Wo, TO* __restrict__ y, int8_t* __restrict__ arg) {
  const unsigned n_out = (unsigned)((long)N * Ho * Wo * C);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int wo = (int)(t % (unsigned)Wo);
    t /= (unsigned)Wo;
    const int ho = (int)(t % (unsigned)Ho), n = (int)(t / (unsigned)Ho);
    float best = -INFINITY;
    int bi = 0;
    for (int ky = 0; ky < k; ++ky) {
      const int h = ho * s - p + ky;
      if (h < 0 || h >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int w = wo * s - p + kx;
        if (w < 0 || w >= W) continue;
        const float v = x[(((long)n * H + h) * W + w) * C + c];
        if (v > best || isnan(v)) {
          best = v;
          bi = ky * k + kx;
          if (isnan(v)) break;
        }
      }
    }
    m_store(y + i, best);
    arg[i] = (int8_t)bi;
  }
}

template <typename TI = float>
__global__ void maxpool_bwd_kernel(const TI* __restrict__ dy, const int8_t* __restrict__ arg, int N, int H, int W,
                                   int C, int k, int s, int p, int Ho, int Wo, float* __restrict__ dx) {
  const unsigned n_in = (unsigned)((long)N * H * W * C);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), n = (int)(t / (unsigned)H);
    float acc = 0.f;
    const int ho_lo = max(0, (h + p - k + s) / s), ho_hi = min(Ho - 1, (h + p) / s);
    const int wo_lo = max(0, (w + p - k + s) / s), wo_hi = min(Wo - 1, (w + p) / s);
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      const int ky = h + p - ho * s;
      if (ky < 0 || ky >= k) continue;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        const int kx = w + p - wo * s;
        if (kx < 0 || kx >= k) continue;
        const long o = (((long)n * Ho + ho) * Wo + wo) * C + c;
        if (arg[o] == ky * k + kx) acc += m_f32(dy[o]);
      }
    }
    dx[i] = acc;
  }
}

// 4-channel forms (C % 4 == 0): float4 / char4 accesses, one index decomposition per 4 channels
// (the stem max-pool at S1 moves 1.2 GB in and 0.3 GB out per launch; the scalar forms ran at ~1.5
// and ~0.9 TB/s)
typedef char char4v __attribute__((ext_vector_type(4)));
template <typename TO = float>
__global__ void maxpool_fwd4_kernel(const float* __restrict__ x, int N, int H, int W, int C4, int k, int s, int p,
                                    int Ho, int Wo, TO* __restrict__ y, int8_t* __restrict__ arg) {
  const unsigned n_out = (unsigned)((long)N * Ho * Wo * C4);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int wo = (int)(t % (unsigned)Wo);
    t /= (unsigned)Wo;
    const int ho = (int)(t % (unsigned)Ho), n = (int)(t / (unsigned)Ho);
    f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bi[4] = {0, 0, 0, 0};
    for (int ky = 0; ky < k; ++ky) {
      const int h = ho * s - p + ky;
      if (h < 0 || h >= H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int w = wo * s - p + kx;
        if (w < 0 || w >= W) continue;
        const f32x4 v = *(const f32x4*)(x + ((((long)n * H + h) * W + w) * C4 + c4) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v[j] > best[j] || isnan(v[j])) {  // first maximum; NaN propagates (torch's max_pool2d rule)
            best[j] = v[j];
            bi[j] = ky * k + kx;
          }
      }
    }
    q4_store(y + (size_t)i * 4, best);  // (rounding commutes with the max: bf16 maps store bf16(max))
    const char4v a = {(char)bi[0], (char)bi[1], (char)bi[2], (char)bi[3]};
    *(char4v*)(arg + (size_t)i * 4) = a;
  }
}

template <typename TI = float>
__global__ void maxpool_bwd4_kernel(const TI* __restrict__ dy, const int8_t* __restrict__ arg, int N, int H, int W,
                                    int C4, int k, int s, int p, int Ho, int Wo, float* __restrict__ dx) {
  const unsigned n_in = (unsigned)((long)N * H * W * C4);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), n = (int)(t / (unsigned)H);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int ho_lo = max(0, (h + p - k + s) / s), ho_hi = min(Ho - 1, (h + p) / s);
    const int wo_lo = max(0, (w + p - k + s) / s), wo_hi = min(Wo - 1, (w + p) / s);
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      const int ky = h + p - ho * s;
      if (ky < 0 || ky >= k) continue;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        const int kx = w + p - wo * s;
        if (kx < 0 || kx >= k) continue;
        const long o = (((long)n * Ho + ho) * Wo + wo) * C4 + c4;
        const char4v a = *(const char4v*)(arg + o * 4);
        const f32x4 g = q4_f32(q4_load(dy + o * 4));
        const int tap = ky * k + kx;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (a[j] == tap) acc[j] += g[j];
      }
    }
    *(f32x4*)(dx + (size_t)i * 4) = acc;
  }
}

// AvgPool2d(k, stride k) / AdaptiveAvgPool2d(1) (k = H = W): y[n,ho,wo,c] = mean of the k x k block
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, int k, int Ho, int Wo,
                                   float* __restrict__ y) {
  const unsigned n_out = (unsigned)((long)N * Ho * Wo * C);
  const float inv = 1.0f / (float)(k * k);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int wo = (int)(t % (unsigned)Wo);
    t /= (unsigned)Wo;
    const int ho = (int)(t % (unsigned)Ho), n = (int)(t / (unsigned)Ho);
    float s = 0.f;
    for (int ky = 0; ky < k; ++ky)
      for (int kx = 0; kx < k; ++kx) s += x[(((long)n * H + ho * k + ky) * W + wo * k + kx) * C + c];
    y[i] = s * inv;
  }
}
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, int N, int H, int W, int C, int k, int Ho, int Wo,
                                   float* __restrict__ dx, int accumulate) {
  const unsigned n_in = (unsigned)((long)N * H * W * C);
  const float inv = 1.0f / (float)(k * k);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), n = (int)(t / (unsigned)H);
    const float v = dy[(((long)n * Ho + h / k) * Wo + w / k) * C + c] * inv;
    dx[i] = accumulate ? dx[i] + v : v;
  }
}

// 4-channel forms over fp32 or bf16 maps (C % 4 == 0): TI / TO = input / output element type
template <typename TI, typename TO>
__global__ void avgpool_fwd4_kernel(const TI* __restrict__ x, int N, int H, int W, int C4, int k, int Ho, int Wo,
                                    TO* __restrict__ y) {
  const unsigned n_out = (unsigned)((long)N * Ho * Wo * C4);
  const float inv = 1.0f / (float)(k * k);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int wo = (int)(t % (unsigned)Wo);
    t /= (unsigned)Wo;
    const int ho = (int)(t % (unsigned)Ho), n = (int)(t / (unsigned)Ho);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < k; ++ky)
      for (int kx = 0; kx < k; ++kx)
        s += q4_f32(q4_load(x + ((((long)n * H + ho * k + ky) * W + wo * k + kx) * C4 + c4) * 4));
    q4_store(y + (size_t)i * 4, s * inv);
  }
}
template <typename TI, typename TO>
__global__ void avgpool_bwd4_kernel(const TI* __restrict__ dy, int N, int H, int W, int C4, int k, int Ho, int Wo,
                                    TO* __restrict__ dx, int accumulate) {
  const unsigned n_in = (unsigned)((long)N * H * W * C4);
  const float inv = 1.0f / (float)(k * k);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), n = (int)(t / (unsigned)H);
    f32x4 v = q4_f32(q4_load(dy + ((((long)n * Ho + h / k) * Wo + w / k) * C4 + c4) * 4)) * inv;
    if (accumulate) v += q4_f32(q4_load(dx + (size_t)i * 4));
    q4_store(dx + (size_t)i * 4, v);
  }
}
template <typename T>
__global__ void upsample_add_fwd4_kernel(const T* __restrict__ base, const T* __restrict__ src, int N, int H, int W,
                                         int C4, int s, T* __restrict__ out) {
  const int h2 = H / s, w2 = W / s;
  const unsigned n = (unsigned)((long)N * H * W * C4);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), nn = (int)(t / (unsigned)H);
    q4_store(out + (size_t)i * 4, q4_f32(q4_load(base + (size_t)i * 4)) +
                                      q4_f32(q4_load(src + ((((long)nn * h2 + h / s) * w2 + w / s) * C4 + c4) * 4)));
  }
}
template <typename T>
__global__ void upsample_bwd4_kernel(const T* __restrict__ dout, int N, int H, int W, int C4, int s,
                                     T* __restrict__ dsrc) {
  const int h2 = H / s, w2 = W / s;
  const unsigned n = (unsigned)((long)N * h2 * w2 * C4);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (unsigned)C4);
    unsigned t = i / (unsigned)C4;
    const int ws = (int)(t % (unsigned)w2);
    t /= (unsigned)w2;
    const int hs = (int)(t % (unsigned)h2), nn = (int)(t / (unsigned)h2);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int dy = 0; dy < s; ++dy)
      for (int dx = 0; dx < s; ++dx) a += q4_f32(q4_load(dout + ((((long)nn * H + hs * s + dy) * W + ws * s + dx) * C4 + c4) * 4));
    q4_store(dsrc + (size_t)i * 4, a);
  }
}

// out = base + nearest-upsample(src, x s)
__global__ void upsample_add_fwd_kernel(const float* __restrict__ base, const float* __restrict__ src, int N, int H,
                                        int W, int C, int s, float* __restrict__ out) {
  const int h2 = H / s, w2 = W / s;
  const unsigned n = (unsigned)((long)N * H * W * C);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int w = (int)(t % (unsigned)W);
    t /= (unsigned)W;
    const int h = (int)(t % (unsigned)H), nn = (int)(t / (unsigned)H);
    out[i] = base[i] + src[(((long)nn * h2 + h / s) * w2 + w / s) * C + c];
  }
}
// dsrc[n, hs, ws, c] = sum of dout over the s x s block
__global__ void upsample_bwd_kernel(const float* __restrict__ dout, int N, int H, int W, int C, int s,
                                    float* __restrict__ dsrc) {
  const int h2 = H / s, w2 = W / s;
  const unsigned n = (unsigned)((long)N * h2 * w2 * C);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = (int)(i % (unsigned)C);
    unsigned t = i / (unsigned)C;
    const int ws = (int)(t % (unsigned)w2);
    t /= (unsigned)w2;
    const int hs = (int)(t % (unsigned)h2), nn = (int)(t / (unsigned)h2);
    float a = 0.f;
    for (int dy = 0; dy < s; ++dy)
      for (int dx = 0; dx < s; ++dx) a += dout[(((long)nn * H + hs * s + dy) * W + ws * s + dx) * C + c];
    dsrc[i] = a;
  }
}

// ---- FCUDown tokens: out[n][0] = 2 x_t[n][0]; out[n][1+p] = gelu(LN(pooled[n][p])) + x_t[n][1+p]
// (the `x_st + x_t` of ConvTransBlock: x_st's cls row is x_t[:, 0] itself, code/models/conformer.py
// :176-177,345).  One wave per row, D <= 1024; saves mean / rstd per row.
template <int NJ>  // 64-column slots per lane: D <= 64 NJ; the row stays in registers (one read of pooled / x_t)
__global__ __launch_bounds__(256) void fcu_down_fwd_kernel(const float* __restrict__ pooled, const float* __restrict__ xt,
                                                           const float* __restrict__ gam, const float* __restrict__ bet,
                                                           float* __restrict__ out, float* __restrict__ mean,
                                                           float* __restrict__ rstd, int N, int np, int D, float eps) {
  const int wv = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const int T = np + 1;
  if (wv >= N * T) return;
  const int n = wv / T, tk = wv % T;
  const float* xr = xt + (long)wv * D;
  float* orow = out + (long)wv * D;
  float xv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
    xv[j] = c < D ? xr[c] : 0.f;
  }
  if (tk == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (j * 64 + lane < D) orow[j * 64 + lane] = 2.f * xv[j];
    return;
  }
  const float* pr = pooled + ((long)n * np + tk - 1) * D;
  float pv[NJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
    pv[j] = c < D ? pr[c] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j * 64 + lane < D) s += pv[j];
  const float mu = warp_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (j * 64 + lane < D) {
      const float d = pv[j] - mu;
      q = fmaf(d, d, q);
    }
  const float rs = 1.0f / sqrtf(warp_sum(q) / (float)D + eps);
  if (lane == 0) {
    mean[(long)n * np + tk - 1] = mu;
    rstd[(long)n * np + tk - 1] = rs;
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
    if (c < D) {
      const float z = (pv[j] - mu) * rs * gam[c] + bet[c];
      orow[c] = 0.5f * z * (1.0f + erff(z * 0.70710678118654752f)) + xv[j];
    }
  }
}

// backward: dxt = dout (cls row doubled); dpooled = LN backward of dout * gelu'(z); per-block
// partial gamma / beta gradients partial[block][0..D) / [D..2D).  A wave owns a row at a time with
// its D/64 columns per lane in registers (D <= 1024): the row's gelu'(z) and xhat are computed once,
// and the gamma / beta partials stay in registers until one LDS reduction over the 4 waves at the end.
constexpr int FCU_NJ = 16;  // D <= 1024
// workgroups of the backward (2048 for large maps: up to 8 waves per SIMD at NJ = 6)
inline int fcu_bwd_blocks(int rows) { return rows < 8192 ? (rows + 3) / 4 : 2048; }
template <int NJ>  // 64-column slots per lane: D <= 64 NJ (the unused slots are predicated off)
__global__ __launch_bounds__(256) void fcu_down_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ pooled,
                                                           const float* __restrict__ gam, const float* __restrict__ bet,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ dxt, float* __restrict__ dpooled,
                                                           float* __restrict__ partial, int N, int np, int D,
                                                           int rows_per_block, int dxt_acc) {
  extern __shared__ float pg[];  // [4 waves][2 * D]
  const int T = np + 1, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float ga[NJ], be[NJ], pgw[NJ], pbw[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
    ga[j] = c < D ? gam[c] : 0.f;
    be[j] = c < D ? bet[c] : 0.f;
    pgw[j] = pbw[j] = 0.f;
  }
  const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, N * T);
  // the next row's dout / pooled values are loaded while this row computes (registers nd / np_), so a
  // wave's rows do not each wait a full memory latency
  float nd[NJ], npv[NJ];
  auto load_row = [&](int row) {
    const int n = row / T, tk = row - n * T;
    const float* dr = dout + (long)row * D;
    const float* pr = pooled + ((long)n * np + (tk > 0 ? tk - 1 : 0)) * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      nd[j] = c < D ? dr[c] : 0.f;
      npv[j] = (c < D && tk > 0) ? pr[c] : 0.f;
    }
  };
  if (r0 + wv < r1) load_row(r0 + wv);
  for (int row = r0 + wv; row < r1; row += 4) {
    const int n = row / T, tk = row - n * T;
    float* xr = dxt + (long)row * D;
    float d[NJ], pvv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      d[j] = nd[j];
      pvv[j] = npv[j];
    }
    if (row + 4 < r1) load_row(row + 4);
    if (tk == 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (j * 64 + lane < D) xr[j * 64 + lane] = dxt_acc ? xr[j * 64 + lane] + 2.f * d[j] : 2.f * d[j];
      continue;
    }
    const long pi = (long)n * np + tk - 1;
    const float mu = mean[pi], rs = rstd[pi];
    float xh[NJ], gz[NJ];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      if (c < D) {
        xr[c] = dxt_acc ? xr[c] + d[j] : d[j];
        xh[j] = (pvv[j] - mu) * rs;
        const float z = xh[j] * ga[j] + be[j];
        const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752f));
        gz[j] = d[j] * fmaf(z, 0.39894228040143268f * __expf(-0.5f * z * z), cdf);
        pgw[j] = fmaf(gz[j], xh[j], pgw[j]);
        pbw[j] += gz[j];
        const float gx = gz[j] * ga[j];
        s1 += gx;
        s2 = fmaf(gx, xh[j], s2);
      } else {
        xh[j] = gz[j] = 0.f;
      }
    }
    s1 = warp_sum(s1) / (float)D;
    s2 = warp_sum(s2) / (float)D;
    float* dp = dpooled + pi * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = j * 64 + lane;
      if (c < D) dp[c] = rs * (gz[j] * ga[j] - s1 - xh[j] * s2);
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = j * 64 + lane;
    if (c < D) {
      pg[wv * 2 * D + c] = pgw[j];
      pg[wv * 2 * D + D + c] = pbw[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += blockDim.x)
    partial[(long)blockIdx.x * 2 * D + c] = (pg[c] + pg[2 * D + c]) + (pg[4 * D + c] + pg[6 * D + c]);
}

__global__ void tokens_cls_set_kernel(float* __restrict__ xt, int N, int T, int D, const float* __restrict__ cls) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * D) return;
  const int n = (int)(i / D), c = (int)(i % D);
  xt[(long)n * T * D + c] = cls[c];
}

// row groups of the per-channel reductions: ~64 rows each, at most 1024 (4 workgroups per CU)
// ---- the 3-channel 7x7 / stride-2 / pad-3 stem (Conformer.conv1 code/models/conformer.py:313-315,
// timm resnet18's conv1) on NHWC fp32 images, 64 output channels: specialised forward and weight
// gradient.  The generic kernels above gather one 4-byte tap per thread per 16-deep K step for this
// conv (Cin = 3 is not 4-aligned) and re-load the 37.6 KB weight per 64-pixel tile; here a tile is a
// 64-pixel segment of one output row, its 7 input rows (133 pixels x 3 channels each, zero-padded) are
// staged into LDS with coalesced row loads, and persistent workgroups keep W^T in LDS across tiles.
// K' = (ky, kx, ci) with ci fastest = ky*21 + kx*3 + ci -- conv_fwd_kernel's K order -- padded to 148;
// v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, so the forward is bit-identical to
// conv_fwd_kernel's.  A tap (ky, kx, ci) of output pixel p sits at float 6p + kx*3 + ci of staged row ky.
constexpr int STEM_PX = 64;     // output pixels per tile
constexpr int STEM_K = 148;     // 147 taps x channels + one zero row (the MFMA's K step is 4)
constexpr int STEM_RF = 399;    // floats per staged input row: (2 * STEM_PX + 5) pixels x 3 channels
constexpr int STEM_ROWF = 400;  // LDS row stride
constexpr int STEM_LD = 80;     // LDS row stride of the [k'][co] / [pixel][co] images: 80 = 16 mod 32
                                // puts lanes 16-31 (the next k / pixel) on the other half of the banks

// the 7 input rows of output row `ho`, pixels [wo0, wo0 + 64): As[ky][3 * j + ci] =
// x[n][2 ho - 3 + ky][2 wo0 - 3 + j][ci] (0 outside the image).  Loaded into registers (STEM_PRE per
// thread) one tile ahead and stored into LDS after the previous tile's MFMAs, so the global latency
// hides behind the matrix work.
constexpr int STEM_PRE = (7 * STEM_RF + 255) / 256;  // 11
__device__ __forceinline__ void stem_load_rows(float (&r)[STEM_PRE], const float* __restrict__ x, int n, int ho, int wo0,
                                               int H, int W) {
  const int wlo = 2 * wo0 - 3;
#pragma unroll
  for (int j = 0; j < STEM_PRE; ++j) {
    const int i = threadIdx.x + 256 * j;
    const int ky = i / STEM_RF, f = i - ky * STEM_RF;
    const int hi = 2 * ho - 3 + ky, wi = wlo + f / 3;
    r[j] = (i < 7 * STEM_RF && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W)
               ? x[(((long)n * H + hi) * W) * 3 + (long)wlo * 3 + f]
               : 0.f;
  }
}
__device__ __forceinline__ void stem_store_rows(float* As, const float (&r)[STEM_PRE]) {
#pragma unroll
  for (int j = 0; j < STEM_PRE; ++j) {
    const int i = threadIdx.x + 256 * j;
    if (i < 7 * STEM_RF) {
      const int ky = i / STEM_RF;
      As[ky * STEM_ROWF + (i - ky * STEM_RF)] = r[j];
    }
  }
}
struct StemTile {
  int n, ho, wo0;
  __device__ StemTile(int t, int Ho, int tpr) {
    const int seg = t % tpr, row = t / tpr;
    ho = row % Ho;
    n = row / Ho;
    wo0 = seg * STEM_PX;
  }
};

__global__ __launch_bounds__(256, 2) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int N,
                                                          int H, int W, int Ho, int Wo, long syn, long syh, long syw,
                                                          int accumulate) {
  __shared__ float Bs[STEM_K * STEM_LD];  // W^T [k'][co]
  __shared__ float As[7 * STEM_ROWF];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < STEM_K * 64; i += 256) {
    const int kp = i >> 6, co = i & 63;
    float v = 0.f;
    if (kp < 147) {
      const int ky = kp / 21, r = kp - ky * 21, kx = r / 3, ci = r - kx * 3;
      v = w[co * 147 + ci * 49 + ky * 7 + kx];
    }
    Bs[kp * STEM_LD + co] = v;
  }
  const int tpr = (Wo + STEM_PX - 1) / STEM_PX, ntiles = N * Ho * tpr;
  const int pr = lane & 15, kl = lane >> 4;
  const int p = wv * 16 + pr;  // this lane's A row (output pixel in the tile)
  float bv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bv[c] = bias ? bias[c * 16 + pr] : 0.f;
  float pre[STEM_PRE];
  if (blockIdx.x < ntiles) {
    const StemTile t0(blockIdx.x, Ho, tpr);
    stem_load_rows(pre, x, t0.n, t0.ho, t0.wo0, H, W);
  }
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const StemTile tt(t, Ho, tpr);
    const int ho = tt.ho, n = tt.n, wo0 = tt.wo0;
    __syncthreads();  // the previous tile's reads of As (and, first time round, the W^T writes)
    stem_store_rows(As, pre);
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) {  // the next tile's rows in flight during this tile's MFMAs
      const StemTile tn(t + gridDim.x, Ho, tpr);
      stem_load_rows(pre, x, tn.n, tn.ho, tn.wo0, H, W);
    }
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < STEM_K / 4; ++ks) {
      const int kp = ks * 4 + kl;
      const int ky = kp / 21, r = kp - ky * 21;
      const float a = kp < 147 ? As[ky * STEM_ROWF + 6 * p + r] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kp * STEM_LD + c * 16 + pr], acc[c], 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int wo = wo0 + wv * 16 + 4 * kl + q;
      if (wo >= Wo) continue;
      float* yr = y + n * syn + ho * syh + wo * syw;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = acc[c][q] + bv[c];
        yr[c * 16 + pr] = accumulate ? yr[c * 16 + pr] + v : v;
      }
    }
  }
}

// weight gradient partials P[block][co][k'] = sum over the block's tiles' pixels of dy[pix][co] x
// im2col[pix][k']: A = dy^T (rows co, k = pixel) from an LDS image of the tile's 64 dy rows, B = the
// staged input rows (cols k', k = pixel); wave w owns co rows [16w, 16w + 16) x all 148 k' (10 tiles).
__global__ __launch_bounds__(256, 2) void stem_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ P, int N, int H, int W, int Ho, int Wo,
                                                         long syn, long syh, long syw) {
  __shared__ float Ds[STEM_PX * STEM_LD];  // dy [pixel][co]
  __shared__ float As[7 * STEM_ROWF];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pr = lane & 15, kl = lane >> 4;
  int off[10];
  bool ok[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const int kp = j * 16 + pr, ky = kp / 21, r = kp - ky * 21;
    ok[j] = kp < 147;
    off[j] = ok[j] ? ky * STEM_ROWF + r : 0;
  }
  f32x4 acc[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tpr = (Wo + STEM_PX - 1) / STEM_PX, ntiles = N * Ho * tpr;
  float pre[STEM_PRE];
  f32x4 dpre[4];  // 64 pixels x 64 channels of dy = 1,024 float4s, 4 per thread
  auto load_dy = [&](const StemTile& tt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + 256 * j, px = i >> 4, c4 = (i & 15) * 4;
      dpre[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (tt.wo0 + px < Wo) dpre[j] = *(const f32x4*)(dy + tt.n * syn + tt.ho * syh + (long)(tt.wo0 + px) * syw + c4);
    }
  };
  if (blockIdx.x < ntiles) {
    const StemTile t0(blockIdx.x, Ho, tpr);
    stem_load_rows(pre, x, t0.n, t0.ho, t0.wo0, H, W);
    load_dy(t0);
  }
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    __syncthreads();
    stem_store_rows(As, pre);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + 256 * j;
      *(f32x4*)(Ds + (i >> 4) * STEM_LD + (i & 15) * 4) = dpre[j];
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) {  // the next tile's operands in flight during this tile's MFMAs
      const StemTile tn(t + gridDim.x, Ho, tpr);
      stem_load_rows(pre, x, tn.n, tn.ho, tn.wo0, H, W);
      load_dy(tn);
    }
#pragma unroll 2
    for (int s = 0; s < STEM_PX / 4; ++s) {
      const int px = 4 * s + kl;
      const float a = Ds[px * STEM_LD + wv * 16 + pr];
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        const float b = ok[j] ? As[off[j] + 6 * px] : 0.f;
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
      }
    }
  }
  // acc[j][q]: co = 16 wv + 4 kl + q, k' = 16 j + pr
  float* out = P + (long)blockIdx.x * 64 * 147;
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(wv * 16 + 4 * kl + q) * 147 + j * 16 + pr] = acc[j][q];
  }
}

// dw[co][ci][ky][kx] (+)= sum_b P[b][co][k'], k' = ky*21 + kx*3 + ci.  A block owns 64 outputs; its 4 waves
// each sum a quarter of the slabs (4 chains), combined in a fixed order through LDS (deterministic).
__global__ __launch_bounds__(256) void stem_dw_reduce_kernel(const float* __restrict__ P, float* __restrict__ dw, int S,
                                                             int accumulate) {
  __shared__ float part[4][64];
  const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + o;
  const int b0 = (S * q) / 4, b1 = (S * (q + 1)) / 4;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < 64 * 147) {
    int b = b0;
    for (; b + 4 <= b1; b += 4) {
      s0 += P[(long)b * 9408 + i];
      s1 += P[(long)(b + 1) * 9408 + i];
      s2 += P[(long)(b + 2) * 9408 + i];
      s3 += P[(long)(b + 3) * 9408 + i];
    }
    for (; b < b1; ++b) s0 += P[(long)b * 9408 + i];
  }
  part[q][o] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q != 0 || i >= 64 * 147) return;
  const float v = (part[0][o] + part[1][o]) + (part[2][o] + part[3][o]);
  const int co = i / 147, kp = i - co * 147, ky = kp / 21, r = kp - ky * 21, kx = r / 3, ci = r - kx * 3;
  float* d = dw + co * 147 + ci * 49 + ky * 7 + kx;
  *d = accumulate ? *d + v : v;
}

// the stem kernels' preconditions: 3 -> 64 channels, 7x7 / 2 / 3, NHWC-contiguous fp32 images, channel-
// contiguous output rows
inline bool stem_ok(const ConvGeom& g) {
  return g.Cin == 3 && g.Cout == 64 && g.kh == 7 && g.kw == 7 && g.stride == 2 && g.pad == 3 && g.sxc == 1 &&
         g.sxw == 3 && g.sxh == 3L * g.W && g.sxn == 3L * g.W * g.H && g.syw >= 64 && g.syw % 4 == 0 &&
         g.syh % 4 == 0 && g.syn % 4 == 0;
}
constexpr int STEM_GRID = 512;  // two 256-thread workgroups per CU (launch_bounds(256, 2))
int g_stem_kernels = 1;  // es_set_stem_kernels: 0 = the generic kernels for the stem too (A/B, tests)
inline bool stem_generic() { return g_stem_kernels == 0; }

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int grid1d(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

ConvGeom make_geom(int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc, int Cout, int kh, int kw,
                   int stride, int pad, long syn, long syh, long syw) {
  ConvGeom g;
  g.N = N; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.kh = kh; g.kw = kw; g.stride = stride; g.pad = pad;
  g.Ho = (H + 2 * pad - kh) / stride + 1;
  g.Wo = (W + 2 * pad - kw) / stride + 1;
  g.sxn = sxn; g.sxh = sxh; g.sxw = sxw; g.sxc = sxc;
  g.syn = syn; g.syh = syh; g.syw = syw;
  return g;
}

bool geom_ok(const ConvGeom& g) {
  return g.N > 0 && g.H > 0 && g.W > 0 && g.Cin > 0 && g.Cout > 0 && g.kh > 0 && g.kw > 0 && g.stride > 0 &&
         g.pad >= 0 && g.Ho > 0 && g.Wo > 0;
}

template <int V_>
int launch_conv_fwd(const float* x, const float* w, const float* bias, float* y, const ConvGeom& g, int accumulate,
                    hipStream_t stream) {
  const int M = g.N * g.Ho * g.Wo;
  if (g.Cout <= 16) {
    hipLaunchKernelGGL((conv_fwd_kernel<256, 16, V_>), dim3((M + 255) / 256, (g.Cout + 15) / 16), 256, 0, stream, x,
                       w, bias, y, g, accumulate);
  } else if (g.Cout <= 32) {
    hipLaunchKernelGGL((conv_fwd_kernel<128, 32, V_>), dim3((M + 127) / 128, (g.Cout + 31) / 32), 256, 0, stream, x,
                       w, bias, y, g, accumulate);
  } else {
    hipLaunchKernelGGL((conv_fwd_kernel<64, 64, V_>), dim3((M + 63) / 64, (g.Cout + 63) / 64), 256, 0, stream, x, w,
                       bias, y, g, accumulate);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <int V_>
int launch_conv_dx(const float* dy, const float* w, float* dx, const ConvGeom& g, int accumulate, hipStream_t stream) {
  const int st = g.stride;
  const int Mq = g.N * ((g.H + st - 1) / st) * ((g.W + st - 1) / st);  // largest phase
  const unsigned ph = (unsigned)(st * st);
  if (g.Cin <= 16) {
    hipLaunchKernelGGL((conv_dx_kernel<256, 16, V_>), dim3((Mq + 255) / 256, (g.Cin + 15) / 16, ph), 256, 0, stream,
                       dy, w, dx, g, accumulate);
  } else if (g.Cin <= 32) {
    hipLaunchKernelGGL((conv_dx_kernel<128, 32, V_>), dim3((Mq + 127) / 128, (g.Cin + 31) / 32, ph), 256, 0, stream,
                       dy, w, dx, g, accumulate);
  } else {
    hipLaunchKernelGGL((conv_dx_kernel<64, 64, V_>), dim3((Mq + 63) / 64, (g.Cin + 63) / 64, ph), 256, 0, stream, dy,
                       w, dx, g, accumulate);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// ---- BatchNorm2d over the global batch (SyncBatchNorm across ranks) -------------------------
__global__ void bn_mean_from_sum_kernel(const float* __restrict__ sum_g, float rows_g, int C, float* __restrict__ mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mean[c] = sum_g[c] / rows_g;
}
// mean / biased var from the global sums; running stats with the unbiased var; rstd saved
__global__ void bn_finalize_global_kernel(const float* __restrict__ sum_g, const float* __restrict__ sq_g, float rows_g,
                                          int C, float eps, float momentum, float* __restrict__ mean,
                                          float* __restrict__ rstd, float* __restrict__ run_mean,
                                          float* __restrict__ run_var, int64_t* __restrict__ nbt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;  // num_batches_tracked: one thread of the launch (no launch of its own)
  if (c >= C) return;
  const float mu = sum_g[c] / rows_g, var = sq_g[c] / rows_g;
  mean[c] = mu;
  rstd[c] = 1.0f / sqrtf(var + eps);
  const float unb = rows_g > 1.f ? sq_g[c] / (rows_g - 1.f) : var;
  run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
  run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
}

// dbeta (+)= local sum g, dgamma (+)= local sum g xhat (sums_local = [sum g | sum g xhat])
__global__ void bn_param_grads_kernel(const float* __restrict__ sums_local, int C, float* __restrict__ dgamma,
                                      float* __restrict__ dbeta, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  dbeta[c] = accumulate ? dbeta[c] + sums_local[c] : sums_local[c];
  dgamma[c] = accumulate ? dgamma[c] + sums_local[C + c] : sums_local[C + c];
}


// ---- host launchers templated on the map element type T (float or bf16); the extern "C" entry points
// below pick T from their flags (bit 0: the maps are bf16) -------------------------------------------
template <typename T>
bool map_v4(int C, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
            const void* e = nullptr) {
  return C % 4 == 0 && al16(a) && (!b || al16(b)) && (!c || al16(c)) && (!d || al16(d)) && (!e || al16(e));
}

template <typename T>
void bn_apply_launch(bool v4, const T* x, long n, int C, const float* mu, const float* rs, const float* rv, float eps,
                     const float* gamma, const float* beta, const T* res, int relu, T* y, hipStream_t stream) {
  constexpr int CVEC = sizeof(T) == 2 ? 8 : 4;  // 16-byte map accesses
  if (g_bn_cs && v4 && C % CVEC == 0) {
    const long nv = n / CVEC;
    hipLaunchKernelGGL((bn_apply_cs_kernel<CVEC, T>), cs_grid(nv, C / CVEC), 256, 0, stream, x, (int)nv, C / CVEC, mu,
                       rs, rv, eps, gamma, beta, res, relu, y);
    return;
  }
  if (v4)
    hipLaunchKernelGGL((bn_apply_kernel<4, T>), grid1d(n / 4), 256, 0, stream, x, (int)(n / 4), C / 4, mu, rs, rv, eps,
                       gamma, beta, res, relu, y);
  else
    hipLaunchKernelGGL((bn_apply_kernel<1, T>), grid1d(n), 256, 0, stream, x, (int)n, C, mu, rs, rv, eps, gamma, beta,
                       res, relu, y);
}

template <int MODE, typename T>
void chan_partial_launch(bool v4, int G, const T* v, RowMap rm, int rows, int C, int per, const float* mean,
                         const float* rstd, const T* dy, const T* y, int relu, float* ws, hipStream_t stream,
                         const float* gamma = nullptr, const float* beta = nullptr) {
  // es_set_bn_sum8(1): the maps summed in 8-channel groups (bf16: 16-byte loads): another fp32 summation order of
  // the same channel sums (a thread's rows and the row-lane count change), kept as a test knob -- round 5 measured
  // no gain -- so that the trainer-level parity bars are checked against a legitimate reordering
  if (g_bn_sum8 && v4 && C % 8 == 0 && rm.sn % 8 == 0 && rm.sp % 8 == 0) {
    if (MODE == 2 && relu && !y)
      hipLaunchKernelGGL((chan_partial_kernel<MODE, 8, T, true>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd,
                         dy, y, relu, ws, gamma, beta);
    else
      hipLaunchKernelGGL((chan_partial_kernel<MODE, 8, T>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd, dy, y,
                         relu, ws, nullptr, nullptr);
    return;
  }
  if (MODE == 2 && relu && !y) {  // the mask rebuilt from x (gamma / beta)
    if (v4)
      hipLaunchKernelGGL((chan_partial_kernel<MODE, 4, T, true>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd,
                         dy, y, relu, ws, gamma, beta);
    else
      hipLaunchKernelGGL((chan_partial_kernel<MODE, 1, T, true>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd,
                         dy, y, relu, ws, gamma, beta);
    return;
  }
  if (v4)
    hipLaunchKernelGGL((chan_partial_kernel<MODE, 4, T>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd, dy, y, relu,
                       ws, nullptr, nullptr);
  else
    hipLaunchKernelGGL((chan_partial_kernel<MODE, 1, T>), G, 256, 0, stream, v, rm, rows, C, per, mean, rstd, dy, y, relu,
                       ws, nullptr, nullptr);
}

template <typename T>
int chan_sum_impl(const T* v, int rows, int C, long sn, long sp, int HW, float* workspace, float* out, int accumulate,
                  hipStream_t stream) {
  if (!v || !out || !workspace) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || HW <= 0) return ES_BAD_SHAPE;
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{sn, sp, HW};
  chan_partial_launch<0, T>(C % 4 == 0 && sn % 4 == 0 && sp % 4 == 0 && al16(v), G, v, rm, rows, C, per, nullptr,
                            nullptr, nullptr, nullptr, 0, workspace, stream);
  ChanFin f{out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, accumulate};
  hipLaunchKernelGGL(chan_final_kernel<0>, (C + 15) / 16, 256, 0, stream, workspace, G, C, f);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_fwd_impl(const T* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                  float* running_var, void* num_batches_tracked, float momentum, float eps, int train, const T* res,
                  int relu, T* y, float* mean, float* rstd, float* workspace, hipStream_t stream) {
  if (!x || !gamma || !beta || !y || !running_mean || !running_var) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0) return ES_BAD_SHAPE;
  const long n = (long)rows * C;
  if (n >= (1L << 31)) return ES_BAD_SHAPE;
  const bool v4 = map_v4<T>(C, x, y, res, gamma, beta) && al16(running_mean) && al16(running_var) &&
                  (!mean || al16(mean)) && (!rstd || al16(rstd));
  if (!train) {
    bn_apply_launch<T>(v4, x, n, C, running_mean, nullptr, running_var, eps, gamma, beta, res, relu, y, stream);
    return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
  }
  if (!mean || !rstd || !workspace) return ES_BAD_ARG;
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{(long)rows * C, (long)C, rows};
  const dim3 fg((C + 15) / 16);
  ChanFin fm{mean, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, 0};
  ChanFin fv{rstd, nullptr, nullptr, mean, running_mean, running_var, eps, momentum, rows, 0, 0,
             (int64_t*)num_batches_tracked};
  chan_partial_launch<0, T>(v4, G, x, rm, rows, C, per, nullptr, nullptr, nullptr, nullptr, 0, workspace, stream);
  hipLaunchKernelGGL(chan_final_kernel<1>, fg, 256, 0, stream, workspace, G, C, fm);
  chan_partial_launch<1, T>(v4, G, x, rm, rows, C, per, mean, nullptr, nullptr, nullptr, 0, workspace, stream);
  hipLaunchKernelGGL(chan_final_kernel<2>, fg, 256, 0, stream, workspace, G, C, fv);
  bn_apply_launch<T>(v4, x, n, C, mean, rstd, nullptr, eps, gamma, beta, res, relu, y, stream);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// the backward's apply pass (dx, optional gout); true when the channel-stationary kernel took it
template <typename T>
bool bn_bwd_apply_cs_launch(bool v4, bool rebuild, const T* x, const T* dy, const T* y, int relu, long n, int C,
                            int rows, const float* mean, const float* rstd, const float* gamma, const float* sums, T* dx,
                            T* gout, const float* beta, hipStream_t stream) {
  constexpr int CVEC = sizeof(T) == 2 ? 8 : 4;
  if (!g_bn_cs || !v4 || C % CVEC) return false;
  const long nv = n / CVEC;
  const int g = cs_grid(nv, C / CVEC);
  if (rebuild)
    hipLaunchKernelGGL((bn_bwd_apply_cs_kernel<CVEC, T, true>), g, 256, 0, stream, x, dy, y, relu, (int)nv, C / CVEC,
                       rows, mean, rstd, gamma, sums, dx, gout, beta);
  else
    hipLaunchKernelGGL((bn_bwd_apply_cs_kernel<CVEC, T, false>), g, 256, 0, stream, x, dy, y, relu, (int)nv, C / CVEC,
                       rows, mean, rstd, gamma, sums, dx, gout, beta);
  return true;
}

// y == null with relu: the mask rebuilt from x (train mode, no residual; beta required)
template <typename T>
int bn2d_bwd_impl(const T* x, const T* y, const T* dy, int rows, int C, int relu, const float* gamma, const float* mean,
                  const float* rstd, int train, const float* running_var, float eps, T* dx, T* gout, float* dgamma,
                  float* dbeta, int accumulate, float* workspace, hipStream_t stream, const float* beta = nullptr) {
  if (!x || !dy || !dx || !gamma || (relu && !y && (!beta || !train))) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0) return ES_BAD_SHAPE;
  const long n = (long)rows * C;
  if (n >= (1L << 31)) return ES_BAD_SHAPE;
  if (!train) {
    if (!running_var) return ES_BAD_ARG;
    hipLaunchKernelGGL(bn_bwd_eval_kernel<T>, grid1d(n), 256, 0, stream, dy, y, relu, n, C, running_var, eps, gamma, dx,
                       gout);
    return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
  }
  if (!mean || !rstd || !workspace || !dgamma || !dbeta) return ES_BAD_ARG;
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{(long)rows * C, (long)C, rows};
  float* sums = workspace + (size_t)G * 2 * C;  // [2C]: sum g, sum g xhat
  const bool v4 = map_v4<T>(C, x, dy, y, dx, gout) && al16(mean) && al16(rstd) && al16(gamma) && al16(sums) &&
                  (!beta || al16(beta));
  chan_partial_launch<2, T>(v4, G, x, rm, rows, C, per, mean, rstd, dy, y, relu, workspace, stream, gamma, beta);
  // sums[0..C) = sum g -> dbeta, sums[C..2C) = sum g xhat -> dgamma
  ChanFin f{dbeta, dgamma, sums, nullptr, nullptr, nullptr, 0.f, 0.f, rows, C, accumulate};
  hipLaunchKernelGGL(chan_final_kernel<3>, (2 * C + 15) / 16, 256, 0, stream, workspace, G, 2 * C, f);
  const bool rebuild = relu && !y;
  if (bn_bwd_apply_cs_launch<T>(v4, rebuild, x, dy, y, relu, n, C, rows, mean, rstd, gamma, sums, dx, gout,
                                rebuild ? beta : nullptr, stream))
    ;
  else if (v4 && rebuild)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<4, T, true>), grid1d(n / 4), 256, 0, stream, x, dy, y, relu, (int)(n / 4),
                       C / 4, rows, mean, rstd, gamma, sums, dx, gout, beta);
  else if (rebuild)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<1, T, true>), grid1d(n), 256, 0, stream, x, dy, y, relu, (int)n, C, rows,
                       mean, rstd, gamma, sums, dx, gout, beta);
  else if (v4)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<4, T>), grid1d(n / 4), 256, 0, stream, x, dy, y, relu, (int)(n / 4), C / 4,
                       rows, mean, rstd, gamma, sums, dx, gout, nullptr);
  else
    hipLaunchKernelGGL((bn_bwd_apply_kernel<1, T>), grid1d(n), 256, 0, stream, x, dy, y, relu, (int)n, C, rows, mean,
                       rstd, gamma, sums, dx, gout, nullptr);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_sums_impl(const T* x, int rows, int C, int mode, const float* sum_g, int rows_g, float* out, float* workspace,
                   hipStream_t stream) {
  if (!x || !out || !workspace || (mode == 1 && !sum_g)) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || (mode != 0 && mode != 1) || (mode == 1 && rows_g <= 0)) return ES_BAD_SHAPE;
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{(long)rows * C, (long)C, rows};
  float* mean = workspace + (size_t)G * 2 * C;  // [C] (the tail es_bn2d_bwd keeps for its sums)
  const bool v4 = C % 4 == 0 && al16(x) && al16(mean);
  if (mode == 1)
    hipLaunchKernelGGL(bn_mean_from_sum_kernel, (C + 255) / 256, 256, 0, stream, sum_g, (float)rows_g, C, mean);
  if (mode == 0)
    chan_partial_launch<0, T>(v4, G, x, rm, rows, C, per, mean, nullptr, nullptr, nullptr, 0, workspace, stream);
  else
    chan_partial_launch<1, T>(v4, G, x, rm, rows, C, per, mean, nullptr, nullptr, nullptr, 0, workspace, stream);
  ChanFin f{out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, 0};
  hipLaunchKernelGGL(chan_final_kernel<0>, (C + 15) / 16, 256, 0, stream, workspace, G, C, f);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_fwd_global_impl(const T* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, void* num_batches_tracked, float momentum, float eps, const float* sum_g,
                         const float* sq_g, int rows_g, const T* res, int relu, T* y, float* mean, float* rstd,
                         hipStream_t stream) {
  if (!x || !gamma || !beta || !running_mean || !running_var || !sum_g || !sq_g || !y || !mean || !rstd)
    return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || rows_g < rows) return ES_BAD_SHAPE;
  const long n = (long)rows * C;
  if (n >= (1L << 31)) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(bn_finalize_global_kernel, (C + 255) / 256, 256, 0, stream, sum_g, sq_g, (float)rows_g, C, eps,
                     momentum, mean, rstd, running_mean, running_var, (int64_t*)num_batches_tracked);
  if (y) {
    const bool v4 = map_v4<T>(C, x, y, res, gamma, beta) && al16(mean) && al16(rstd);
    bn_apply_launch<T>(v4, x, n, C, mean, rstd, nullptr, eps, gamma, beta, res, relu, y, stream);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_fwd_partials_impl(const T* x, int rows, int C, float* partials, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, void* num_batches_tracked, float momentum, float eps,
                           const T* res, int relu, T* y, float* mean, float* rstd, hipStream_t stream) {
  // y == NULL (no residual): the statistics, running buffers and mean / rstd only -- a bf16 conv applies the
  // normalisation as it gathers this map (es_conv2d_fwd_bf16_bnin_ex)
  if (!x || !partials || !gamma || !beta || !running_mean || !running_var || (!y && res) || !mean || !rstd)
    return ES_BAD_ARG;
  if (rows <= 0 || C <= 0) return ES_BAD_SHAPE;
  const long n = (long)rows * C;
  if (n >= (1L << 31)) return ES_BAD_SHAPE;
  const int nblk = (rows + 127) / 128, G = 64;
  float* P = partials;  // level 1 overwrites group-leading slots in place
  if (nblk > G) {
    const int ng = (nblk + G - 1) / G;
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<false>, dim3((C + 63) / 64, ng), 256, 0, stream, P, nblk, 128, 1,
                       G, rows, C, C, eps, momentum, mean, rstd, running_mean, running_var, nullptr);
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<true>, dim3((C + 63) / 64, 1), 256, 0, stream, P, ng, 128 * G, G,
                       ng, rows, C, C, eps, momentum, mean, rstd, running_mean, running_var, (int64_t*)num_batches_tracked);
  } else {
    hipLaunchKernelGGL(bn_stats_from_partials_kernel<true>, dim3((C + 63) / 64, 1), 256, 0, stream, P, nblk, 128, 1,
                       nblk, rows, C, C, eps, momentum, mean, rstd, running_mean, running_var, (int64_t*)num_batches_tracked);
  }
  if (y) {
    const bool v4 = map_v4<T>(C, x, y, res, gamma, beta) && al16(mean) && al16(rstd);
    bn_apply_launch<T>(v4, x, n, C, mean, rstd, nullptr, eps, gamma, beta, res, relu, y, stream);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_bwd_sums_impl(const T* x, const T* y, const T* dy, int rows, int C, int relu, const float* mean,
                       const float* rstd, float* out, float* workspace, hipStream_t stream) {
  if (!x || !dy || !mean || !rstd || !out || !workspace || (relu && !y)) return ES_BAD_ARG;
  if (rows <= 0 || C <= 0) return ES_BAD_SHAPE;
  const int G = chan_groups(rows);
  const int per = (rows + G - 1) / G;
  const RowMap rm{(long)rows * C, (long)C, rows};
  const bool v4 = map_v4<T>(C, x, dy, y) && al16(mean) && al16(rstd);
  chan_partial_launch<2, T>(v4, G, x, rm, rows, C, per, mean, rstd, dy, y, relu, workspace, stream);
  ChanFin f{out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, rows, 0, 0};
  hipLaunchKernelGGL(chan_final_kernel<0>, (2 * C + 15) / 16, 256, 0, stream, workspace, G, 2 * C, f);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

template <typename T>
int bn2d_bwd_global_impl(const T* x, const T* y, const T* dy, int rows, int C, int relu, const float* gamma,
                         const float* mean, const float* rstd, const float* sums_local, const float* sums_g, int rows_g,
                         T* dx, T* gout, float* dgamma, float* dbeta, int accumulate, hipStream_t stream) {
  if (!x || !dy || !gamma || !mean || !rstd || !sums_local || !sums_g || !dx || !dgamma || !dbeta || (relu && !y))
    return ES_BAD_ARG;
  if (rows <= 0 || C <= 0 || rows_g < rows) return ES_BAD_SHAPE;
  const long n = (long)rows * C;
  if (n >= (1L << 31)) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(bn_param_grads_kernel, (C + 255) / 256, 256, 0, stream, sums_local, C, dgamma, dbeta, accumulate);
  const bool v4 = map_v4<T>(C, x, dy, y, dx, gout) && al16(mean) && al16(rstd) && al16(gamma) && al16(sums_g);
  if (v4)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<4, T>), grid1d(n / 4), 256, 0, stream, x, dy, y, relu, (int)(n / 4), C / 4,
                       rows_g, mean, rstd, gamma, sums_g, dx, gout);
  else
    hipLaunchKernelGGL((bn_bwd_apply_kernel<1, T>), grid1d(n), 256, 0, stream, x, dy, y, relu, (int)n, C, rows_g, mean,
                       rstd, gamma, sums_g, dx, gout);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

// flags of the map entry points: bit 0 = the (input) maps are bf16; pools / upsampling: bit 1 = the output
// map is bf16 (bit 0 the input)
constexpr int MAPS_BF16 = 1, OUT_BF16 = 2;

}  // namespace

extern "C" {

// 1 (default): the specialised stem kernels for 3 -> 64 channel 7x7 / 2 / 3 convs on NHWC images;
// 0: the generic implicit-GEMM kernels (bit-identical forward).  Returns the previous value.
// tuning knob: 1 (default) = the channel-stationary BatchNorm apply kernels (parameters loaded once per thread,
// 16-byte map accesses) where the channel count allows, 0 = the per-iteration forms (bit-identical); returns the
// previous value, or ES_BAD_ARG (unchanged) for any other value
int es_set_bn_cs(int v) {
  if (v != 0 && v != 1) return ES_BAD_ARG;
  const int old = g_bn_cs;
  g_bn_cs = v;
  return old;
}

// test knob: 1 = the BatchNorm channel sums (chan_partial_kernel) over 8-channel groups (a different fp32
// summation order of the same sums), 0 (default) = 4-channel groups; returns the previous value, or ES_BAD_ARG
// (unchanged) for any other value
int es_set_bn_sum8(int v) {
  if (v != 0 && v != 1) return ES_BAD_ARG;
  const int old = g_bn_sum8;
  g_bn_sum8 = v;
  return old;
}

int es_set_stem_kernels(int v) {
  const int old = g_stem_kernels;
  g_stem_kernels = v;
  return old;
}

// y[n, ho, wo, co] (+)= conv(x)  (Conv2d, groups = 1).  x at element strides (sxn, sxh, sxw, sxc),
// y at (syn, syh, syw) with channel stride 1.  Ho = (H + 2p - kh) / s + 1.
int es_conv2d_fwd(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                  const float* w, const float* bias, int Cout, int kh, int kw, int stride, int pad, float* y, long syn,
                  long syh, long syw, int accumulate, hipStream_t stream) {
  if (!x || !w || !y) return ES_BAD_ARG;
  const ConvGeom g = make_geom(N, H, W, Cin, sxn, sxh, sxw, sxc, Cout, kh, kw, stride, pad, syn, syh, syw);
  if (!geom_ok(g)) return ES_BAD_SHAPE;
  if (stem_ok(g) && al16(y) && !stem_generic()) {
    const int tiles = N * g.Ho * ((g.Wo + STEM_PX - 1) / STEM_PX);
    hipLaunchKernelGGL(stem_fwd_kernel, std::min(tiles, STEM_GRID), 256, 0, stream, x, w, bias, y, N, H, W, g.Ho, g.Wo,
                       syn, syh, syw, accumulate);
    return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
  }
  const bool v4 = Cin % 4 == 0 && sxc == 1 && sxw % 4 == 0 && sxh % 4 == 0 && sxn % 4 == 0 && al16(x);
  return v4 ? launch_conv_fwd<4>(x, w, bias, y, g, accumulate, stream)
            : launch_conv_fwd<1>(x, w, bias, y, g, accumulate, stream);
}

// dx (+)= conv^T(dy): the data gradient, written at dx's element strides (sxn, sxh, sxw, sxc)
int es_conv2d_bwd_data(const float* dy, long syn, long syh, long syw, const float* w, int N, int H, int W, int Cin,
                       int Cout, int kh, int kw, int stride, int pad, float* dx, long sxn, long sxh, long sxw, long sxc,
                       int accumulate, hipStream_t stream) {
  if (!dy || !w || !dx) return ES_BAD_ARG;
  const ConvGeom g = make_geom(N, H, W, Cin, sxn, sxh, sxw, sxc, Cout, kh, kw, stride, pad, syn, syh, syw);
  if (!geom_ok(g)) return ES_BAD_SHAPE;
  const bool v4 = Cout % 4 == 0 && syw % 4 == 0 && syh % 4 == 0 && syn % 4 == 0 && al16(dy);
  return v4 ? launch_conv_dx<4>(dy, w, dx, g, accumulate, stream) : launch_conv_dx<1>(dy, w, dx, g, accumulate, stream);
}

// workgroup tiles per pixel split of es_conv2d_bwd_weight (callers size `splits` from it)
int es_conv2d_dw_tiles(int Cout, int Cin, int kh, int kw) {
  const int K = Cin * kh * kw;
  if (Cout <= 32) return (K + 63) / 64;
  if (K <= 32) return (Cout + 63) / 64;
  return ((Cout + 63) / 64) * ((K + 63) / 64);
}

size_t es_conv2d_bwd_weight_workspace(int Cout, int Cin, int kh, int kw, int splits) {
  return (size_t)splits * Cout * Cin * kh * kw;
}

// dw[co, ci, ky, kx] (+)= sum over output pixels of dy x im2col(x); `splits` pixel ranges reduced
// through workspace (es_conv2d_bwd_weight_workspace floats)
int es_conv2d_bwd_weight(const float* x, int N, int H, int W, int Cin, long sxn, long sxh, long sxw, long sxc,
                         const float* dy, long syn, long syh, long syw, int Cout, int kh, int kw, int stride, int pad,
                         int splits, float* workspace, float* dw, int accumulate, hipStream_t stream) {
  if (!x || !dy || !dw || !workspace) return ES_BAD_ARG;
  const ConvGeom g = make_geom(N, H, W, Cin, sxn, sxh, sxw, sxc, Cout, kh, kw, stride, pad, syn, syh, syw);
  if (!geom_ok(g) || splits <= 0) return ES_BAD_SHAPE;
  const int M = N * g.Ho * g.Wo, K = Cin * kh * kw;
  if (stem_ok(g) && al16(dy) && !stem_generic()) {  // partial slabs: one per workgroup
    const int tiles = N * g.Ho * ((g.Wo + STEM_PX - 1) / STEM_PX);
    const int grid = std::min(std::min(tiles, STEM_GRID), splits);  // the caller sized `splits` slabs
    hipLaunchKernelGGL(stem_dw_kernel, grid, 256, 0, stream, x, dy, workspace, N, H, W, g.Ho, g.Wo, syn, syh, syw);
    hipLaunchKernelGGL(stem_dw_reduce_kernel, (64 * 147 + 63) / 64, 256, 0, stream, workspace, dw, grid, accumulate);
    return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
  }
  int chunk = (M + splits - 1) / splits;
  chunk = (chunk + CBK - 1) / CBK * CBK;
  const int S = (M + chunk - 1) / chunk;
  // 64-column tiles (K' = Cin k^2 is 64..2304 here; wider tiles left most of a small conv's tile empty);
  // rows sized to Cout (es_conv2d_dw_tiles mirrors this choice for split sizing)
  if (Cout <= 16) {
    hipLaunchKernelGGL((conv_dw_kernel<16, 64>), dim3((Cout + 15) / 16, (K + 63) / 64, S), 256, 0, stream, x, dy,
                       workspace, g, chunk);
  } else if (Cout <= 32) {
    hipLaunchKernelGGL((conv_dw_kernel<32, 64>), dim3((Cout + 31) / 32, (K + 63) / 64, S), 256, 0, stream, x, dy,
                       workspace, g, chunk);
  } else if (K <= 16) {  // 1x1 conv from 16 channels
    hipLaunchKernelGGL((conv_dw_kernel<64, 16>), dim3((Cout + 63) / 64, 1, S), 256, 0, stream, x, dy, workspace, g,
                       chunk);
  } else if (K <= 32) {
    hipLaunchKernelGGL((conv_dw_kernel<64, 32>), dim3((Cout + 63) / 64, 1, S), 256, 0, stream, x, dy, workspace, g,
                       chunk);
  } else {
    hipLaunchKernelGGL((conv_dw_kernel<64, 64>), dim3((Cout + 63) / 64, (K + 63) / 64, S), 256, 0, stream, x, dy,
                       workspace, g, chunk);
  }
  const long n = (long)Cout * K;
  if (S >= 32) {  // many slabs: 16 lanes per column over the slabs
    ChanFin f{dw, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0, 0, accumulate};
    hipLaunchKernelGGL(chan_final_kernel<0>, (unsigned)((n + 15) / 16), 256, 0, stream, workspace, S, (int)n, f);
  } else {
    hipLaunchKernelGGL(sum_slabs_kernel, grid1d(n), 256, 0, stream, workspace, dw, S, n, accumulate);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

size_t es_chan_workspace(int rows, int C) {
  const int G = chan_groups(rows);
  return (size_t)G * 2 * C + 2 * C;
}

// out[c] (+)= sum over rows of v; row r at (r / HW) * sn + (r % HW) * sp (bias gradients)
int es_chan_sum(const float* v, int rows, int C, long sn, long sp, int HW, float* workspace, float* out,
                int accumulate, hipStream_t stream) {
  return chan_sum_impl<float>(v, rows, C, sn, sp, HW, workspace, out, accumulate, stream);
}
// es_chan_sum over an fp32 (flags 0) or bf16 (flags 1) map
int es_chan_sum_ex(const void* v, int rows, int C, long sn, long sp, int HW, float* workspace, float* out,
                   int accumulate, int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  return flags ? chan_sum_impl<bf16>((const bf16*)v, rows, C, sn, sp, HW, workspace, out, accumulate, stream)
               : chan_sum_impl<float>((const float*)v, rows, C, sn, sp, HW, workspace, out, accumulate, stream);
}

// BatchNorm2d over x [rows = N*H*W, C] (NHWC contiguous).  train: batch mean / biased variance,
// running stats updated with momentum (unbiased variance) and num_batches_tracked += 1 (nullable);
// mean / rstd saved for the backward.  eval: running statistics.  y = bn(x) (+ res) then ReLU if relu.
int es_bn2d_fwd(const float* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                float* running_var, void* num_batches_tracked, float momentum, float eps, int train, const float* res,
                int relu, float* y, float* mean, float* rstd, float* workspace, hipStream_t stream) {
  return bn2d_fwd_impl<float>(x, rows, C, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                              train, res, relu, y, mean, rstd, workspace, stream);
}
// es_bn2d_fwd with x / res / y as fp32 (flags 0) or bf16 (flags 1) maps: statistics and the affine map in
// fp32, y rounded once
int es_bn2d_fwd_ex(const void* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, void* num_batches_tracked, float momentum, float eps, int train, const void* res,
                   int relu, void* y, float* mean, float* rstd, float* workspace, int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_fwd_impl<bf16>((const bf16*)x, rows, C, gamma, beta, running_mean, running_var, num_batches_tracked,
                               momentum, eps, train, (const bf16*)res, relu, (bf16*)y, mean, rstd, workspace, stream);
  return bn2d_fwd_impl<float>((const float*)x, rows, C, gamma, beta, running_mean, running_var, num_batches_tracked,
                              momentum, eps, train, (const float*)res, relu, (float*)y, mean, rstd, workspace, stream);
}

// Backward of es_bn2d_fwd (train mode): g = dy * [y > 0 if relu] (written to gout when non-null: the
// gradient of the residual input), dx = BN backward of g, dgamma (+)= sum g xhat, dbeta (+)= sum g.
// eval mode (train = 0): dx = g * gamma / sqrt(running_var + eps), no parameter gradients.
int es_bn2d_bwd(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* gamma,
                const float* mean, const float* rstd, int train, const float* running_var, float eps, float* dx,
                float* gout, float* dgamma, float* dbeta, int accumulate, float* workspace, hipStream_t stream) {
  return bn2d_bwd_impl<float>(x, y, dy, rows, C, relu, gamma, mean, rstd, train, running_var, eps, dx, gout, dgamma,
                              dbeta, accumulate, workspace, stream);
}
// es_bn2d_bwd with x / y / dy / dx / gout as fp32 (flags 0) or bf16 (flags 1) maps (sums in fp32)
int es_bn2d_bwd_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* gamma,
                   const float* mean, const float* rstd, int train, const float* running_var, float eps, void* dx,
                   void* gout, float* dgamma, float* dbeta, int accumulate, float* workspace, int flags,
                   hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_bwd_impl<bf16>((const bf16*)x, (const bf16*)y, (const bf16*)dy, rows, C, relu, gamma, mean, rstd, train,
                               running_var, eps, (bf16*)dx, (bf16*)gout, dgamma, dbeta, accumulate, workspace, stream);
  return bn2d_bwd_impl<float>((const float*)x, (const float*)y, (const float*)dy, rows, C, relu, gamma, mean, rstd,
                              train, running_var, eps, (float*)dx, (float*)gout, dgamma, dbeta, accumulate, workspace,
                              stream);
}

// ---- SyncBatchNorm2d (the Conformer's BatchNorm2d over the global batch at N > 1) ------------
// Per-channel sums of an NHWC map [rows, C] (contiguous):  mode 0: out[c] = sum x;  mode 1:
// out[c] = sum (x - sum_g[c] / rows_g)^2, centred on the GLOBAL mean (sum_g = the all-reduced mode-0
// sums).  workspace: es_chan_workspace(rows, C) floats.
int es_bn2d_sums(const float* x, int rows, int C, int mode, const float* sum_g, int rows_g, float* out,
                 float* workspace, hipStream_t stream) {
  return bn2d_sums_impl<float>(x, rows, C, mode, sum_g, rows_g, out, workspace, stream);
}
int es_bn2d_sums_ex(const void* x, int rows, int C, int mode, const float* sum_g, int rows_g, float* out,
                    float* workspace, int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  return flags ? bn2d_sums_impl<bf16>((const bf16*)x, rows, C, mode, sum_g, rows_g, out, workspace, stream)
               : bn2d_sums_impl<float>((const float*)x, rows, C, mode, sum_g, rows_g, out, workspace, stream);
}

// Train-mode BatchNorm2d from the global sums (sum_g, centred sq_g over rows_g rows): mean / rstd
// saved, running stats updated (unbiased variance over rows_g), num_batches_tracked += 1 (nullable),
// y = bn(x) (+ res) then ReLU if relu -- es_bn2d_fwd with the statistics of every rank's rows.
int es_bn2d_fwd_global(const float* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, void* num_batches_tracked, float momentum, float eps, const float* sum_g,
                       const float* sq_g, int rows_g, const float* res, int relu, float* y, float* mean, float* rstd,
                       hipStream_t stream) {
  return bn2d_fwd_global_impl<float>(x, rows, C, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
                                     eps, sum_g, sq_g, rows_g, res, relu, y, mean, rstd, stream);
}
int es_bn2d_fwd_global_ex(const void* x, int rows, int C, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, void* num_batches_tracked, float momentum, float eps, const float* sum_g,
                          const float* sq_g, int rows_g, const void* res, int relu, void* y, float* mean, float* rstd,
                          int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_fwd_global_impl<bf16>((const bf16*)x, rows, C, gamma, beta, running_mean, running_var,
                                      num_batches_tracked, momentum, eps, sum_g, sq_g, rows_g, (const bf16*)res, relu,
                                      (bf16*)y, mean, rstd, stream);
  return bn2d_fwd_global_impl<float>((const float*)x, rows, C, gamma, beta, running_mean, running_var,
                                     num_batches_tracked, momentum, eps, sum_g, sq_g, rows_g, (const float*)res, relu,
                                     (float*)y, mean, rstd, stream);
}

// Train-mode BatchNorm2d whose batch statistics come from the producing conv's per-block partials
// (es_conv2d_fwd_bf16_bnstats: blocks of 128 rows): no statistics pass over x.  Running stats,
// num_batches_tracked, mean / rstd and y = bn(x) (+ res) (relu) as es_bn2d_fwd.
int es_bn2d_fwd_partials(const float* x, int rows, int C, float* partials, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, void* num_batches_tracked,
                         float momentum, float eps, const float* res, int relu, float* y, float* mean, float* rstd,
                         hipStream_t stream) {
  return bn2d_fwd_partials_impl<float>(x, rows, C, partials, gamma, beta, running_mean, running_var,
                                       num_batches_tracked, momentum, eps, res, relu, y, mean, rstd, stream);
}
// es_bn2d_bwd_ex for a train-mode ReLU BatchNorm without residual whose output y was not kept: the ReLU mask is
// rebuilt from x with the forward's affine map and rounding (bn_relu_live), so the backward reads x and dy only
int es_bn2d_bwd_recompute_ex(const void* x, const void* dy, int rows, int C, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta, int accumulate,
                             float* workspace, int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (!beta) return ES_BAD_ARG;
  if (flags)
    return bn2d_bwd_impl<bf16>((const bf16*)x, nullptr, (const bf16*)dy, rows, C, 1, gamma, mean, rstd, 1, nullptr, 0.f,
                               (bf16*)dx, nullptr, dgamma, dbeta, accumulate, workspace, stream, beta);
  return bn2d_bwd_impl<float>((const float*)x, nullptr, (const float*)dy, rows, C, 1, gamma, mean, rstd, 1, nullptr,
                              0.f, (float*)dx, nullptr, dgamma, dbeta, accumulate, workspace, stream, beta);
}
int es_bn2d_fwd_partials_ex(const void* x, int rows, int C, float* partials, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, void* num_batches_tracked, float momentum,
                            float eps, const void* res, int relu, void* y, float* mean, float* rstd, int flags,
                            hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_fwd_partials_impl<bf16>((const bf16*)x, rows, C, partials, gamma, beta, running_mean, running_var,
                                        num_batches_tracked, momentum, eps, (const bf16*)res, relu, (bf16*)y, mean,
                                        rstd, stream);
  return bn2d_fwd_partials_impl<float>((const float*)x, rows, C, partials, gamma, beta, running_mean, running_var,
                                       num_batches_tracked, momentum, eps, (const float*)res, relu, (float*)y, mean,
                                       rstd, stream);
}

// Backward, local half: out[0..C) = sum g, out[C..2C) = sum g xhat over this rank's rows
// (g = dy * [y > 0 if relu]).  workspace: es_chan_workspace(rows, C) floats.
int es_bn2d_bwd_sums(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* mean,
                     const float* rstd, float* out, float* workspace, hipStream_t stream) {
  return bn2d_bwd_sums_impl<float>(x, y, dy, rows, C, relu, mean, rstd, out, workspace, stream);
}
int es_bn2d_bwd_sums_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* mean,
                        const float* rstd, float* out, float* workspace, int flags, hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_bwd_sums_impl<bf16>((const bf16*)x, (const bf16*)y, (const bf16*)dy, rows, C, relu, mean, rstd, out,
                                    workspace, stream);
  return bn2d_bwd_sums_impl<float>((const float*)x, (const float*)y, (const float*)dy, rows, C, relu, mean, rstd, out,
                                   workspace, stream);
}

// Backward, global half: dx = rstd gamma (g - sum_g g / rows_g - xhat sum_g (g xhat) / rows_g) with the
// all-reduced sums (so dx is d(sum of every rank's loss)/dx), gout = g (nullable: the residual
// input's gradient); dgamma / dbeta (+)= this rank's LOCAL sums (the gradient all-reduce averages them).
int es_bn2d_bwd_global(const float* x, const float* y, const float* dy, int rows, int C, int relu, const float* gamma,
                       const float* mean, const float* rstd, const float* sums_local, const float* sums_g, int rows_g,
                       float* dx, float* gout, float* dgamma, float* dbeta, int accumulate, hipStream_t stream) {
  return bn2d_bwd_global_impl<float>(x, y, dy, rows, C, relu, gamma, mean, rstd, sums_local, sums_g, rows_g, dx, gout,
                                     dgamma, dbeta, accumulate, stream);
}
int es_bn2d_bwd_global_ex(const void* x, const void* y, const void* dy, int rows, int C, int relu, const float* gamma,
                          const float* mean, const float* rstd, const float* sums_local, const float* sums_g, int rows_g,
                          void* dx, void* gout, float* dgamma, float* dbeta, int accumulate, int flags,
                          hipStream_t stream) {
  if (flags & ~MAPS_BF16) return ES_BAD_ARG;
  if (flags)
    return bn2d_bwd_global_impl<bf16>((const bf16*)x, (const bf16*)y, (const bf16*)dy, rows, C, relu, gamma, mean, rstd,
                                      sums_local, sums_g, rows_g, (bf16*)dx, (bf16*)gout, dgamma, dbeta, accumulate,
                                      stream);
  return bn2d_bwd_global_impl<float>((const float*)x, (const float*)y, (const float*)dy, rows, C, relu, gamma, mean,
                                     rstd, sums_local, sums_g, rows_g, (float*)dx, (float*)gout, dgamma, dbeta,
                                     accumulate, stream);
}

// MaxPool2d(k, s, p) over NHWC; arg = int8 window index of the (first) maximum.  _ex flags: 2 = y is a
// bf16 map (x stays fp32: the stem's BatchNorm output)
int es_maxpool2d_fwd_ex(const float* x, int N, int H, int W, int C, int k, int s, int p, void* y, void* arg, int flags,
                        hipStream_t stream) {
  if (!x || !y || !arg || (flags & ~OUT_BF16)) return ES_BAD_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || k > 11 || s <= 0 || p < 0 || 2 * p > k) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  const int Ho = (H + 2 * p - k) / s + 1, Wo = (W + 2 * p - k) / s + 1;
  const bool b16 = flags & OUT_BF16;
  if (C % 4 == 0) {
    const int g = grid1d((long)N * Ho * Wo * C / 4);
    if (b16)
      hipLaunchKernelGGL(maxpool_fwd4_kernel<bf16>, g, 256, 0, stream, x, N, H, W, C / 4, k, s, p, Ho, Wo, (bf16*)y,
                         (int8_t*)arg);
    else
      hipLaunchKernelGGL(maxpool_fwd4_kernel<float>, g, 256, 0, stream, x, N, H, W, C / 4, k, s, p, Ho, Wo, (float*)y,
                         (int8_t*)arg);
  } else {
    const int g = grid1d((long)N * Ho * Wo * C);
    if (b16)
      hipLaunchKernelGGL(maxpool_fwd_kernel<bf16>, g, 256, 0, stream, x, N, H, W, C, k, s, p, Ho, Wo, (bf16*)y,
                         (int8_t*)arg);
    else
      hipLaunchKernelGGL(maxpool_fwd_kernel<float>, g, 256, 0, stream, x, N, H, W, C, k, s, p, Ho, Wo, (float*)y,
                         (int8_t*)arg);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_maxpool2d_fwd(const float* x, int N, int H, int W, int C, int k, int s, int p, float* y, void* arg,
                     hipStream_t stream) {
  return es_maxpool2d_fwd_ex(x, N, H, W, C, k, s, p, y, arg, 0, stream);
}

// _ex flags: 1 = dy is a bf16 map (dx stays fp32)
int es_maxpool2d_bwd_ex(const void* dy, const void* arg, int N, int H, int W, int C, int k, int s, int p, float* dx,
                        int flags, hipStream_t stream) {
  if (!dy || !dx || !arg || (flags & ~MAPS_BF16)) return ES_BAD_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || k > 11 || s <= 0 || p < 0) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  const int Ho = (H + 2 * p - k) / s + 1, Wo = (W + 2 * p - k) / s + 1;
  const int8_t* a = (const int8_t*)arg;
  if (C % 4 == 0) {
    const int g = grid1d((long)N * H * W * C / 4);
    if (flags)
      hipLaunchKernelGGL(maxpool_bwd4_kernel<bf16>, g, 256, 0, stream, (const bf16*)dy, a, N, H, W, C / 4, k, s, p, Ho,
                         Wo, dx);
    else
      hipLaunchKernelGGL(maxpool_bwd4_kernel<float>, g, 256, 0, stream, (const float*)dy, a, N, H, W, C / 4, k, s, p,
                         Ho, Wo, dx);
  } else {
    const int g = grid1d((long)N * H * W * C);
    if (flags)
      hipLaunchKernelGGL(maxpool_bwd_kernel<bf16>, g, 256, 0, stream, (const bf16*)dy, a, N, H, W, C, k, s, p, Ho, Wo,
                         dx);
    else
      hipLaunchKernelGGL(maxpool_bwd_kernel<float>, g, 256, 0, stream, (const float*)dy, a, N, H, W, C, k, s, p, Ho,
                         Wo, dx);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_maxpool2d_bwd(const float* dy, const void* arg, int N, int H, int W, int C, int k, int s, int p, float* dx,
                     hipStream_t stream) {
  return es_maxpool2d_bwd_ex(dy, arg, N, H, W, C, k, s, p, dx, 0, stream);
}

// AvgPool2d(kernel k, stride k, no padding) over NHWC (H, W multiples of k).  _ex flags: 1 = x is a bf16
// map, 2 = y is a bf16 map (C % 4 == 0 for any bf16 map)
int es_avgpool2d_fwd_ex(const void* x, int N, int H, int W, int C, int k, void* y, int flags, hipStream_t stream) {
  if (!x || !y || (flags & ~3)) return ES_BAD_ARG;
  if (N <= 0 || C <= 0 || k <= 0 || H % k || W % k || (flags && C % 4)) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  const int Ho = H / k, Wo = W / k;
  if (C % 4 == 0 && al16(x) && al16(y)) {
    const int g = grid1d((long)N * Ho * Wo * C / 4);
#define AVG_F(TI, TO) \
  hipLaunchKernelGGL((avgpool_fwd4_kernel<TI, TO>), g, 256, 0, stream, (const TI*)x, N, H, W, C / 4, k, Ho, Wo, (TO*)y)
    switch (flags) {
      case 0: AVG_F(float, float); break;
      case 1: AVG_F(bf16, float); break;
      case 2: AVG_F(float, bf16); break;
      default: AVG_F(bf16, bf16); break;
    }
#undef AVG_F
  } else {
    if (flags) return ES_BAD_SHAPE;
    hipLaunchKernelGGL(avgpool_fwd_kernel, grid1d((long)N * Ho * Wo * C), 256, 0, stream, (const float*)x, N, H, W, C,
                       k, Ho, Wo, (float*)y);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_avgpool2d_fwd(const float* x, int N, int H, int W, int C, int k, float* y, hipStream_t stream) {
  return es_avgpool2d_fwd_ex(x, N, H, W, C, k, y, 0, stream);
}

// _ex flags: 1 = dy is a bf16 map, 2 = dx is a bf16 map (accumulate: dx (+)=, added in fp32, rounded once)
int es_avgpool2d_bwd_ex(const void* dy, int N, int H, int W, int C, int k, void* dx, int accumulate, int flags,
                        hipStream_t stream) {
  if (!dy || !dx || (flags & ~3)) return ES_BAD_ARG;
  if (N <= 0 || C <= 0 || k <= 0 || H % k || W % k || (flags && C % 4)) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  if (C % 4 == 0 && al16(dy) && al16(dx)) {
    const int g = grid1d((long)N * H * W * C / 4);
#define AVG_B(TI, TO)                                                                                            \
  hipLaunchKernelGGL((avgpool_bwd4_kernel<TI, TO>), g, 256, 0, stream, (const TI*)dy, N, H, W, C / 4, k, H / k, W / k, \
                     (TO*)dx, accumulate)
    switch (flags) {
      case 0: AVG_B(float, float); break;
      case 1: AVG_B(bf16, float); break;
      case 2: AVG_B(float, bf16); break;
      default: AVG_B(bf16, bf16); break;
    }
#undef AVG_B
  } else {
    if (flags) return ES_BAD_SHAPE;
    hipLaunchKernelGGL(avgpool_bwd_kernel, grid1d((long)N * H * W * C), 256, 0, stream, (const float*)dy, N, H, W, C, k,
                       H / k, W / k, (float*)dx, accumulate);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_avgpool2d_bwd(const float* dy, int N, int H, int W, int C, int k, float* dx, int accumulate,
                     hipStream_t stream) {
  return es_avgpool2d_bwd_ex(dy, N, H, W, C, k, dx, accumulate, 0, stream);
}

// out[N, H, W, C] = base + nearest-upsample(src [N, H/s, W/s, C], x s).  _ex flags: 1 = every map bf16
int es_upsample_add_fwd_ex(const void* base, const void* src, int N, int H, int W, int C, int s, void* out, int flags,
                           hipStream_t stream) {
  if (!base || !src || !out || (flags & ~MAPS_BF16)) return ES_BAD_ARG;
  if (N <= 0 || C <= 0 || s <= 0 || H % s || W % s || (flags && C % 4)) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  if (C % 4 == 0 && al16(base) && al16(src) && al16(out)) {
    const int g = grid1d((long)N * H * W * C / 4);
    if (flags)
      hipLaunchKernelGGL(upsample_add_fwd4_kernel<bf16>, g, 256, 0, stream, (const bf16*)base, (const bf16*)src, N, H, W,
                         C / 4, s, (bf16*)out);
    else
      hipLaunchKernelGGL(upsample_add_fwd4_kernel<float>, g, 256, 0, stream, (const float*)base, (const float*)src, N, H,
                         W, C / 4, s, (float*)out);
  } else {
    if (flags) return ES_BAD_SHAPE;
    hipLaunchKernelGGL(upsample_add_fwd_kernel, grid1d((long)N * H * W * C), 256, 0, stream, (const float*)base,
                       (const float*)src, N, H, W, C, s, (float*)out);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_upsample_add_fwd(const float* base, const float* src, int N, int H, int W, int C, int s, float* out,
                        hipStream_t stream) {
  return es_upsample_add_fwd_ex(base, src, N, H, W, C, s, out, 0, stream);
}

// dsrc = block sums of dout (the base's gradient is dout itself).  _ex flags: 1 = both maps bf16
int es_upsample_bwd_ex(const void* dout, int N, int H, int W, int C, int s, void* dsrc, int flags, hipStream_t stream) {
  if (!dout || !dsrc || (flags & ~MAPS_BF16)) return ES_BAD_ARG;
  if (N <= 0 || C <= 0 || s <= 0 || H % s || W % s || (flags && C % 4)) return ES_BAD_SHAPE;
  if ((long)N * H * W * C >= (1L << 31)) return ES_BAD_SHAPE;  // 32-bit index arithmetic in the kernels
  if (C % 4 == 0 && al16(dout) && al16(dsrc)) {
    const int g = grid1d((long)N * (H / s) * (W / s) * C / 4);
    if (flags)
      hipLaunchKernelGGL(upsample_bwd4_kernel<bf16>, g, 256, 0, stream, (const bf16*)dout, N, H, W, C / 4, s,
                         (bf16*)dsrc);
    else
      hipLaunchKernelGGL(upsample_bwd4_kernel<float>, g, 256, 0, stream, (const float*)dout, N, H, W, C / 4, s,
                         (float*)dsrc);
  } else {
    if (flags) return ES_BAD_SHAPE;
    hipLaunchKernelGGL(upsample_bwd_kernel, grid1d((long)N * (H / s) * (W / s) * C), 256, 0, stream,
                       (const float*)dout, N, H, W, C, s, (float*)dsrc);
  }
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}
int es_upsample_bwd(const float* dout, int N, int H, int W, int C, int s, float* dsrc, hipStream_t stream) {
  return es_upsample_bwd_ex(dout, N, H, W, C, s, dsrc, 0, stream);
}


// FCUDown + ConvTransBlock's sum: out [N, np+1, D] (token rows) from pooled [N, np, D] and x_t.
int es_fcu_down_tokens_fwd(const float* pooled, const float* xt, const float* ln_w, const float* ln_b, float* out,
                           float* mean, float* rstd, int N, int np, int D, float eps, hipStream_t stream) {
  if (!pooled || !xt || !ln_w || !ln_b || !out || !mean || !rstd) return ES_BAD_ARG;
  if (N <= 0 || np <= 0 || D <= 0 || D > 64 * FCU_NJ) return ES_BAD_SHAPE;
  const long waves = (long)N * (np + 1);
  const unsigned blocks = (unsigned)((waves + 3) / 4);
  const int nj = (D + 63) / 64;
#define FCU_FWD(NJ_) \
  hipLaunchKernelGGL(fcu_down_fwd_kernel<NJ_>, blocks, 256, 0, stream, pooled, xt, ln_w, ln_b, out, mean, rstd, N, np, D, eps)
  if (nj <= 2) FCU_FWD(2);
  else if (nj <= 4) FCU_FWD(4);
  else if (nj <= 6) FCU_FWD(6);
  else if (nj <= 8) FCU_FWD(8);
  else if (nj <= 12) FCU_FWD(12);
  else FCU_FWD(16);
#undef FCU_FWD
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

size_t es_fcu_down_workspace(int N, int np, int D) {
  return (size_t)fcu_bwd_blocks(N * (np + 1)) * 2 * D;
}

// backward: dxt [N, np+1, D] (overwritten), dpooled [N, np, D] (overwritten), ln_w / ln_b grads (+)=
int es_fcu_down_tokens_bwd_ex(const float* dout, const float* pooled, const float* ln_w, const float* ln_b,
                              const float* mean, const float* rstd, float* dxt, float* dpooled, float* dln_w,
                              float* dln_b, int accumulate, int N, int np, int D, float* workspace, int dxt_accumulate,
                              hipStream_t stream);
int es_fcu_down_tokens_bwd(const float* dout, const float* pooled, const float* ln_w, const float* ln_b,
                           const float* mean, const float* rstd, float* dxt, float* dpooled, float* dln_w,
                           float* dln_b, int accumulate, int N, int np, int D, float* workspace, hipStream_t stream) {
  return es_fcu_down_tokens_bwd_ex(dout, pooled, ln_w, ln_b, mean, rstd, dxt, dpooled, dln_w, dln_b, accumulate, N, np,
                                   D, workspace, 0, stream);
}

// es_fcu_down_tokens_bwd with dxt (+)= (dxt_accumulate: the x_t gradient added to what dxt holds -- the
// second consumer of a gradient sink, conformer._GradSink)
int es_fcu_down_tokens_bwd_ex(const float* dout, const float* pooled, const float* ln_w, const float* ln_b,
                              const float* mean, const float* rstd, float* dxt, float* dpooled, float* dln_w,
                              float* dln_b, int accumulate, int N, int np, int D, float* workspace, int dxt_accumulate,
                              hipStream_t stream) {
  if (!dout || !pooled || !ln_w || !ln_b || !mean || !rstd || !dxt || !dpooled || !dln_w || !dln_b || !workspace)
    return ES_BAD_ARG;
  if (N <= 0 || np <= 0 || D <= 0 || D > 64 * FCU_NJ) return ES_BAD_SHAPE;
  const int rows = N * (np + 1);
  const int blocks = fcu_bwd_blocks(rows);
  const int per = (rows + blocks - 1) / blocks;
  const size_t lds = (size_t)4 * 2 * D * 4;
  const int nj = (D + 63) / 64;
#define FCU_BWD(NJ_)                                                                                           \
  hipLaunchKernelGGL(fcu_down_bwd_kernel<NJ_>, blocks, 256, lds, stream, dout, pooled, ln_w, ln_b, mean, rstd, dxt, \
                     dpooled, workspace, N, np, D, per, dxt_accumulate)
  if (nj <= 2) FCU_BWD(2);
  else if (nj <= 4) FCU_BWD(4);
  else if (nj <= 6) FCU_BWD(6);
  else if (nj <= 8) FCU_BWD(8);
  else if (nj <= 12) FCU_BWD(12);
  else FCU_BWD(16);
#undef FCU_BWD
  // partial[b][0..D) = dgamma, [D..2D) = dbeta
  ChanFin f{dln_w, dln_b, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0, D, accumulate};
  hipLaunchKernelGGL(chan_final_kernel<3>, (2 * D + 15) / 16, 256, 0, stream, workspace, blocks, 2 * D, f);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

int es_tokens_cls_set(float* xt, int N, int T, int D, const float* cls, hipStream_t stream) {
  if (!xt || !cls) return ES_BAD_ARG;
  if (N <= 0 || T <= 0 || D <= 0) return ES_BAD_SHAPE;
  hipLaunchKernelGGL(tokens_cls_set_kernel, (unsigned)(((long)N * D + 255) / 256), 256, 0, stream, xt, N, T, D, cls);
  return hipGetLastError() == hipSuccess ? ES_OK : ES_HIP_ERROR;
}

}  // extern "C"
